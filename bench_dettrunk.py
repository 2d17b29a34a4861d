#!/usr/bin/env python3
"""Timing of the detector's trunk (cosypose_amd.detector_trunk, csrc/kernels_dettrunk.hip) on one GPU, at bench_dethead.py's workload: 8 frames
padded to 800x1088 through ResNet-50 + FPN (256 channels, five levels 200x272 ... 13x17).  Prints one JSON line.
bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 900 python bench_dettrunk.py --out profiles/dettrunk_bench.json

Per storage type (float32, float16): the median WALL time of `--runs` calls of DetectorTrunk (device work and the host's share, synchronised
before and after), and of its three parts alone (stem: pack + GEMM + pool; the four stages; the FPN).  The torch side is the same network
restated below as torch.nn modules on the device in the same dtype (Conv2d, a frozen batch norm, max_pool2d, interpolate), timed the same way
in the same process; for float16 the cast of the input and of the outputs is part of the torch call, as packing is part of ours.  No ratio is
fixed in advance: a part that comes out slower than torch says so (`slower_than_torch_ops`).  `equal`: on a subsample (a 96 x 128 crop of
image 0) the stem, the first 3x3 convolution and the first strided downsample, each run alone, lie within DESIGN.md section 27's
(K + 3) u (|scale| S + |shift|) of a float64 torch evaluation on the CPU fed the operands rounded to the storage type."""
import argparse
import json
import statistics
import time

PEAK_TFLOPS = {'float32': 155.0, 'float16': 2500.0}      # float32 MFMA as measured, 16-bit nominal
U = {'float32': 2.0 ** -24, 'float16': 2.0 ** -23}
PLANES, BLOCKS, FPN_C = (64, 128, 256, 512), (3, 4, 6, 3), 256


def build_backbone(gen):
    import torch
    import torch.nn.functional as F
    from torch import nn

    class FrozenBN(nn.Module):
        def __init__(self, n):
            super().__init__()
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                self.register_buffer(k, torch.ones(n))

        def forward(self, x):
            scale = self.weight * self.running_var.rsqrt()
            return x * scale.reshape(1, -1, 1, 1) + (self.bias - self.running_mean * scale).reshape(1, -1, 1, 1)

    class Block(nn.Module):
        def __init__(self, c_in, planes, stride, down):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(c_in, planes, 1, bias=False), FrozenBN(planes)
            self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), FrozenBN(planes)
            self.conv3, self.bn3 = nn.Conv2d(planes, 4 * planes, 1, bias=False), FrozenBN(4 * planes)
            self.downsample = nn.Sequential(nn.Conv2d(c_in, 4 * planes, 1, stride, bias=False), FrozenBN(4 * planes)) if down else None

        def forward(self, x):
            out = torch.relu(self.bn1(self.conv1(x)))
            out = torch.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return torch.relu(out + (x if self.downsample is None else self.downsample(x)))

    class Body(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), FrozenBN(64)
            c = 64
            for s, (planes, n) in enumerate(zip(PLANES, BLOCKS), 1):
                setattr(self, f'layer{s}', nn.Sequential(*[Block(c if i == 0 else 4 * planes, planes, 2 if (s > 1 and i == 0) else 1, i == 0) for i in range(n)]))
                c = 4 * planes

        def stem(self, x):
            return F.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)

        def stages(self, x):
            out = []
            for s in range(1, 5):
                x = getattr(self, f'layer{s}')(x)
                out.append(x)
            return out

    class FPN(nn.Module):
        def __init__(self):
            super().__init__()
            self.inner_blocks = nn.ModuleList([nn.Conv2d(4 * p, FPN_C, 1) for p in PLANES])
            self.layer_blocks = nn.ModuleList([nn.Conv2d(FPN_C, FPN_C, 3, padding=1) for _ in PLANES])

        def forward(self, feats):
            last = self.inner_blocks[-1](feats[-1])
            out = [self.layer_blocks[-1](last)]
            for l in range(len(feats) - 2, -1, -1):
                lateral = self.inner_blocks[l](feats[l])
                last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode='nearest')
                out.insert(0, self.layer_blocks[l](last))
            return out + [F.max_pool2d(out[-1], 1, 2, 0)]

    class Backbone(nn.Module):
        def __init__(self):
            super().__init__()
            self.body, self.fpn = Body(), FPN()

        def forward(self, x):
            return self.fpn(self.body.stages(self.body.stem(x)))

    m = Backbone()
    for name, p in m.named_parameters():                          # He-style: activations stay O(1) through the 53 layers
        fan_in = p[0].numel() if p.dim() > 1 else 1
        p.data = torch.randn(p.shape, generator=gen) * ((2.0 / fan_in) ** 0.5 if p.dim() > 1 else 0.1)
    for name, b in m.named_buffers():
        if name.endswith('running_var'):
            b.copy_(torch.rand(b.shape, generator=gen) * 1.5 + 0.5)
        elif name.endswith('bn3.weight') or name.endswith('downsample.1.weight'):
            b.copy_((torch.rand(b.shape, generator=gen) + 0.5) * 0.5)
        elif name.endswith('weight'):
            b.copy_(torch.rand(b.shape, generator=gen) + 0.5)
        else:
            b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
    return m.eval().requires_grad_(False)


def flop_counts(B, H, W):
    """multiply-adds x 2 of the stem, the stages and the FPN at (B,3,H,W)"""
    o = lambda n: (n - 1) // 2 + 1
    h, w = o(H), o(W)
    stem = 2.0 * B * h * w * 147 * 64
    h, w, c, stages, sizes = o(h), o(w), 64, 0.0, []
    for s, (planes, n) in enumerate(zip(PLANES, BLOCKS)):
        for i in range(n):
            ho, wo = (o(h), o(w)) if (s > 0 and i == 0) else (h, w)
            stages += 2.0 * B * (h * w * c * planes + ho * wo * 9 * planes * planes + ho * wo * planes * 4 * planes)
            if i == 0:
                stages += 2.0 * B * ho * wo * c * 4 * planes
            h, w, c = ho, wo, 4 * planes
        sizes.append((h, w))
    fpn = sum(2.0 * B * h * w * (4 * p * FPN_C + 9 * FPN_C * FPN_C) for (h, w), p in zip(sizes, PLANES))
    return dict(stem=stem, stages=stages, fpn=fpn, trunk=stem + stages + fpn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1088)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from cosypose_amd import build
    from cosypose_amd.detector_trunk import DetectorTrunk, trunk_conv_layer
    assert torch.cuda.is_available(), 'bench_dettrunk.py needs a ROCm device'
    B, H, W = args.frames, args.height, args.width
    model = build_backbone(torch.Generator().manual_seed(args.seed))
    images = torch.randn((B, 3, H, W), generator=torch.Generator(device='cuda').manual_seed(args.seed), device='cuda')
    flops = flop_counts(B, H, W)

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

    def layer_share(layer, conv, bn, x, dtype):
        """one layer alone on the subsample x (CPU float32) against float64 on the CPU fed the operands rounded to the storage type"""
        td = getattr(torch, dtype)
        rnd = lambda t: t.float().to(td).double()
        scale = (bn.weight * bn.running_var.rsqrt()).double()
        shift = (bn.bias - bn.running_mean * (bn.weight * bn.running_var.rsqrt())).double()
        xr, w = rnd(x), rnd(conv.weight)
        y = F.conv2d(xr, w, None, conv.stride, conv.padding) * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
        S = F.conv2d(xr.abs(), w.abs(), None, conv.stride, conv.padding) * scale.abs().reshape(1, -1, 1, 1) + shift.abs().reshape(1, -1, 1, 1)
        K = w[0].numel() + (5 if w.shape[2] == 7 else 0)
        got = trunk_conv_layer(x.cuda().contiguous(), layer).cpu().double()
        want = torch.relu(y) if layer.relu else y
        return float(((got - want).abs() / ((K + 3) * U[dtype] * S).clamp(min=1e-300)).max()), rnd(want).float()

    results = {}
    with torch.no_grad():
        for dtype in ('float32', 'float16'):
            td = getattr(torch, dtype)
            trunk = DetectorTrunk.from_modules(model, dtype=td, device='cuda')
            dev_model = build_backbone(torch.Generator().manual_seed(args.seed))
            dev_model.load_state_dict(model.state_dict())
            dev_model.to(device='cuda', dtype=td)

            crop = images[:1, :, :96, :128].cpu()
            b0 = model.body.layer1[0]
            share0, x1 = layer_share(trunk.stem, model.body.conv1, model.body.bn1, crop, dtype)
            x1 = F.max_pool2d(x1, 3, 2, 1)
            share1, x2 = layer_share(trunk.block(1, 0).conv1, b0.conv1, b0.bn1, x1, dtype)
            share2, _ = layer_share(trunk.block(1, 0).conv2, b0.conv2, b0.bn2, x2, dtype)
            b1 = model.body.layer2[0]
            x3 = torch.randn((1, 256, 24, 32), generator=torch.Generator().manual_seed(args.seed + 1))
            share3, _ = layer_share(trunk.block(2, 0).downsample, b1.downsample[0], b1.downsample[1], x3, dtype)
            share = max(share0, share1, share2, share3)

            trunk._ready(images.device)
            pooled = trunk.stem_rows(images)
            feats = trunk.stage_rows(pooled[0], B, pooled[1], pooled[2])
            ours = dict(trunk=lambda: trunk(images), stem=lambda: trunk.stem_rows(images), stages=lambda: trunk.stage_rows(pooled[0], B, pooled[1], pooled[2]),
                        fpn=lambda: trunk.fpn_rows(feats, B))
            t_pooled = dev_model.body.stem(images.to(td))
            t_feats = dev_model.body.stages(t_pooled)
            theirs = dict(trunk=lambda: [t.float() for t in dev_model(images.to(td))], stem=lambda: dev_model.body.stem(images.to(td)),
                          stages=lambda: dev_model.body.stages(t_pooled), fpn=lambda: [t.float() for t in dev_model.fpn(t_feats)])
            parts = {}
            for part in ('trunk', 'stem', 'stages', 'fpn'):
                ms, runs = wall(ours[part], args.runs, args.warmup)
                t_ms, t_runs = wall(theirs[part], args.runs, args.warmup)
                tf = flops[part] / ms / 1e9
                parts[part] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, gflop=round(flops[part] / 1e9, 1), tflops=round(tf, 1),
                                   torch_tflops=round(flops[part] / t_ms / 1e9, 1), peak_tflops=PEAK_TFLOPS[dtype], share_of_peak=round(tf / PEAK_TFLOPS[dtype], 4),
                                   speedup_vs_torch_ops=round(t_ms / ms, 2), slower_than_torch_ops=ms > t_ms)
            parts['stem']['share_of_trunk'] = round(parts['stem']['ms'] / parts['trunk']['ms'], 3)
            got, want = trunk(images), dev_model(images.to(td))
            rel = max(float((g - w.float()).abs().max() / w.float().abs().max()) for g, w in zip(got, want))
            results[dtype] = dict(parts=parts, equal=bool(share <= 1.0), largest_share_of_layer_bound=share, max_rel_diff_to_torch_ops=rel,
                                  arena_bytes=trunk.arena_bytes(), stem_cols_bytes=trunk._arena['stem_cols'].numel() * trunk._arena['stem_cols'].element_size())
            del trunk, dev_model, pooled, feats, t_pooled, t_feats, got, want
            torch.cuda.empty_cache()
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector trunk: ResNet-50 + FPN, float32 and float16, sum of the median wall times of one call',
        'value': round(sum(r['parts']['trunk']['ms'] for r in results.values()), 3), 'unit': 'ms', 'higher_is_better': False,
        'torch_ms': round(sum(r['parts']['trunk']['torch_ms'] for r in results.values()), 3),
        'types': results, 'equal': all(r['equal'] for r in results.values()),
        'slower_than_torch_ops': {d: r['parts']['trunk']['slower_than_torch_ops'] for d, r in results.items()},
        'config': {'seed': args.seed, 'frames': B, 'height': H, 'width': W, 'blocks': list(BLOCKS), 'fpn_channels': FPN_C, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Timing of the detector's heads (cosypose_amd.detector_heads, csrc/kernels_dethead.hip) on one GPU, at bench_rpn.py's workload: 8 frames
padded to 800x1088, five FPN levels (200x272 ... 13x17), C = 256 channels, A = 3 anchors per cell.  Prints one JSON line.
bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 900 python bench_dethead.py --out profiles/dethead_bench.json

Three stages per storage type (float32, float16), each the median WALL time of `--runs` calls (device work and the host's share,
synchronised before and after): the RPN head over the five levels; the box head + predictor on 8 x 1000 rows of (256,7,7), hidden width
1024, 22 classes; the mask head + predictor on 800 rows of (256,14,14).  Inputs and outputs are float32 NCHW on both sides.  Each stage is
timed in the same process against the same layers as torch.nn modules on the device in the same dtype (`torch_ms`; for float16 the cast of
the input and of the outputs is part of the torch call, as packing is part of ours).  No ratio is fixed in advance: a stage that comes out
slower than torch says so (`slower_than_torch_ops`).  `tflops`: the stage's multiply-adds x 2 over its time, beside the peaks
(PEAK_TFLOPS).  `equal`: on a subsample (the coarsest level of image 0; 16 RoI rows; 2 mask rows) every output of the head lies within the
running float64 bound of DESIGN.md section 26 of a float64 torch evaluation on the CPU fed the operands rounded to the storage type, AND
every layer, run alone on the float64 chain's value at its input, lies within its own (K + 2) u S (`largest_share_of_layer_bound`): the
running bound alone grows by sum |w| per layer and would let a misplaced cell through."""
import argparse
import json
import statistics
import time

GRID = [(200, 272), (100, 136), (50, 68), (25, 34), (13, 17)]
PEAK_TFLOPS = {'float32': 155.0, 'float16': 2500.0}      # float32 MFMA as measured, 16-bit nominal
U = {'float32': 2.0 ** -24, 'float16': 2.0 ** -23}


def build_modules(C, A, hidden, K, gen):
    import torch
    from torch import nn

    class Rpn(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.cls_logits, self.bbox_pred = nn.Conv2d(C, C, 3, padding=1), nn.Conv2d(C, A, 1), nn.Conv2d(C, 4 * A, 1)

        def forward(self, feats):
            hidden_ = [torch.relu(self.conv(f)) for f in feats]
            return [self.cls_logits(h) for h in hidden_], [self.bbox_pred(h) for h in hidden_]

    class Box(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc6, self.fc7 = nn.Linear(C * 49, hidden), nn.Linear(hidden, hidden)

        def forward(self, x):
            return torch.relu(self.fc7(torch.relu(self.fc6(x.flatten(1)))))

    class BoxPred(nn.Module):
        def __init__(self):
            super().__init__()
            self.cls_score, self.bbox_pred = nn.Linear(hidden, K), nn.Linear(hidden, 4 * K)

        def forward(self, x):
            return self.cls_score(x), self.bbox_pred(x)

    class Mask(nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(1, 5):
                setattr(self, f'mask_fcn{i}', nn.Conv2d(C, C, 3, padding=1))

        def forward(self, x):
            for i in range(1, 5):
                x = torch.relu(getattr(self, f'mask_fcn{i}')(x))
            return x

    class MaskPred(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv5_mask, self.mask_fcn_logits = nn.ConvTranspose2d(C, C, 2, 2), nn.Conv2d(C, K, 1)

        def forward(self, x):
            return self.mask_fcn_logits(torch.relu(self.conv5_mask(x)))

    mods = [Rpn(), Box(), BoxPred(), Mask(), MaskPred()]
    for m in mods:
        for p in m.parameters():                                  # He-style: activations stay O(1) through the chains
            fan_in = p[0].numel() if p.dim() > 1 else 1
            p.data = torch.randn(p.shape, generator=gen) * ((2.0 / fan_in) ** 0.5 if p.dim() > 1 else 0.1)
        m.eval().requires_grad_(False)
    return mods


def bound64(layers, x, dtype):
    """float64 value and running bound of a chain of (kind, weight, bias, relu) on the CPU: section 26's e_out = sum |w| e_in + (K + 2) u (S +
    sum |w| e_in), plus one storage ulp where a 16-bit intermediate is stored; and per layer (input, value, (K + 2) u S) of that layer alone"""
    import torch
    import torch.nn.functional as Fn
    u = U[dtype]
    td = getattr(torch, dtype)
    rnd = lambda t: t.float().to(td).double()

    def apply(kind, w, b, t):
        if kind == 'linear':
            return Fn.linear(t, w, b)
        if kind == 'deconv':
            return Fn.conv_transpose2d(t, w, b, stride=2)
        return Fn.conv2d(t, w, b, padding=w.shape[2] // 2)
    value, err, per_layer = rnd(x.double()), None, []
    for i, (kind, w, b, relu) in enumerate(layers):
        w64, b64 = rnd(w.double()), b.double()
        K = w64[0].numel() if kind != 'deconv' else w64.shape[0]
        y = apply(kind, w64, b64, value)
        S = apply(kind, w64.abs(), b64.abs(), value.abs())
        carried = torch.zeros_like(S) if err is None else apply(kind, w64.abs(), None, err)
        err = carried + (K + 2) * u * (S + carried)
        x_in = rnd(value)                                         # this layer alone, on an input the storage type holds exactly
        y_in, S_in = apply(kind, w64, b64, x_in), apply(kind, w64.abs(), b64.abs(), x_in.abs())
        per_layer.append((x_in, torch.relu(y_in) if relu else y_in, (K + 2) * u * S_in))
        value = torch.relu(y) if relu else y
        if i + 1 < len(layers) and dtype != 'float32':
            mag = (value.abs() + err).clamp(min=2.0 ** -14)
            err = err + 2.0 ** (torch.floor(torch.log2(mag)) - 10)
            value = rnd(value)
    return value, err, per_layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--rois', type=int, default=1000, help='box head rows per frame')
    ap.add_argument('--masks', type=int, default=800, help='mask head rows')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import torch
    from cosypose_amd import build
    from cosypose_amd.detector_heads import DetectorHeads, conv_layer
    assert torch.cuda.is_available(), 'bench_dethead.py needs a ROCm device'
    B, C, A, hidden, K = args.frames, args.channels, 3, 1024, 22
    R, D = B * args.rois, args.masks
    cpu_gen = torch.Generator().manual_seed(args.seed)
    mods = build_modules(C, A, hidden, K, cpu_gen)
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    feats = [torch.randn((B, C, H, W), generator=gen, device='cuda') for H, W in GRID]
    roi = torch.randn((R, C, 7, 7), generator=gen, device='cuda')
    mroi = torch.randn((D, C, 14, 14), generator=gen, device='cuda')
    M = sum(B * H * W for H, W in GRID)
    flops = {'rpn_head': 2.0 * M * (9 * C * C + C * 5 * A), 'box_head': 2.0 * R * (49 * C * hidden + hidden * hidden + hidden * 5 * K),
             'mask_head': 2.0 * D * 196 * (4 * 9 * C * C + C * 4 * C + 4 * C * K)}

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

    rpn_m, box_m, pred_m, mask_m, mpred_m = mods
    sub = dict(
        rpn_head=([('conv', rpn_m.conv.weight, rpn_m.conv.bias, True),
                   ('conv', torch.cat([rpn_m.cls_logits.weight, rpn_m.bbox_pred.weight]), torch.cat([rpn_m.cls_logits.bias, rpn_m.bbox_pred.bias]), False)],
                  feats[-1][:1].cpu()),
        box_head=([('linear', box_m.fc6.weight, box_m.fc6.bias, True), ('linear', box_m.fc7.weight, box_m.fc7.bias, True),
                   ('linear', torch.cat([pred_m.cls_score.weight, pred_m.bbox_pred.weight]), torch.cat([pred_m.cls_score.bias, pred_m.bbox_pred.bias]), False)],
                  roi[:16].flatten(1).cpu()),
        mask_head=([('conv', getattr(mask_m, f'mask_fcn{i}').weight, getattr(mask_m, f'mask_fcn{i}').bias, True) for i in range(1, 5)]
                   + [('deconv', mpred_m.conv5_mask.weight, mpred_m.conv5_mask.bias, True),
                      ('conv', mpred_m.mask_fcn_logits.weight, mpred_m.mask_fcn_logits.bias, False)], mroi[:2].cpu()))

    results = {}
    with torch.no_grad():
        for dtype in ('float32', 'float16'):
            td = getattr(torch, dtype)
            heads = DetectorHeads.from_modules(*mods, dtype=td, device='cuda')
            dev_mods = [type(m)() for m in mods]
            for dm, m in zip(dev_mods, mods):
                dm.load_state_dict(m.state_dict())
                dm.to(device='cuda', dtype=td).eval().requires_grad_(False)
            t_rpn, t_box, t_pred, t_mask, t_mpred = dev_mods

            def ours(stage):
                if stage == 'rpn_head':
                    o, d = heads.rpn_head(feats)
                    return torch.cat([o[-1][:1], d[-1][:1]], 1)
                if stage == 'box_head':
                    c, r = heads.box_head(roi)
                    return torch.cat([c[:16], r[:16]], 1)
                return heads.mask_head(mroi)[:2]

            def theirs(stage):
                if stage == 'rpn_head':
                    o, d = t_rpn([f.to(td) for f in feats])
                    return [t.float() for t in o], [t.float() for t in d]
                if stage == 'box_head':
                    c, r = t_pred(t_box(roi.to(td)))
                    return c.float(), r.float()
                return t_mpred(t_mask(mroi.to(td))).float()

            packed = heads.layers()                               # in the order of the three chains of `sub`
            first = {'rpn_head': 0, 'box_head': 2, 'mask_head': 5}
            stages = {}
            for stage in ('rpn_head', 'box_head', 'mask_head'):
                got = ours(stage).cpu().double()
                want, err, per_layer = bound64(*sub[stage], dtype)
                share = float(((got - want).abs() / err.clamp(min=1e-300)).max())
                # the running bound grows by sum |w| per layer and hides a misplaced cell; so every layer is also run alone on the subsample,
                # fed the float64 chain's value at its input (rounded to the storage type on the way in), and held to its own (K + 2) u S
                layer_share = 0.0
                for n, (x_in, y, bound) in enumerate(per_layer):
                    out = conv_layer(x_in.float().cuda().contiguous(), packed[first[stage] + n]).cpu().double()
                    layer_share = max(layer_share, float(((out - y).abs() / bound.clamp(min=1e-300)).max()))
                ms, runs = wall(lambda: ours(stage), args.runs, args.warmup)
                t_ms, t_runs = wall(lambda: theirs(stage), args.runs, args.warmup)
                tf = flops[stage] / ms / 1e9
                stages[stage] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, equal=bool(share <= 1.0 and layer_share <= 1.0), largest_share_of_bound=share,
                                     largest_share_of_layer_bound=layer_share,
                                     max_abs_err=float((got - want).abs().max()), gflop=round(flops[stage] / 1e9, 1), tflops=round(tf, 1),
                                     torch_tflops=round(flops[stage] / t_ms / 1e9, 1), peak_tflops=PEAK_TFLOPS[dtype],
                                     share_of_peak=round(tf / PEAK_TFLOPS[dtype], 4), speedup_vs_torch_ops=round(t_ms / ms, 2),
                                     slower_than_torch_ops=ms > t_ms)
            results[dtype] = stages
            del heads, dev_mods
            torch.cuda.empty_cache()
    stamp = build.read_stamp() or {}
    total = round(sum(s['ms'] for st in results.values() for s in st.values()), 3)
    result = {
        'metric': 'detector heads: RPN head + box head + mask head, float32 and float16, sum of the median wall times',
        'value': total, 'unit': 'ms', 'higher_is_better': False,
        'torch_ms': round(sum(s['torch_ms'] for st in results.values() for s in st.values()), 3),
        'stages': results, 'equal': all(s['equal'] for st in results.values() for s in st.values()),
        'config': {'seed': args.seed, 'frames': B, 'levels': [list(g) for g in GRID], 'anchors_per_cell': A, 'channels': C, 'box_rows': R,
                   'hidden': hidden, 'classes': K, 'mask_rows': D, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

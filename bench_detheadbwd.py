#!/usr/bin/env python3
"""Timing of the detector heads' training step (forward + backward of cosypose_amd.detector_heads with trainable=True, csrc/kernels_dethead.hip
and csrc/kernels_detbwd.hip) on one GPU, float32, at bench_dethead.py's shapes: 8 frames padded to 800x1088, five FPN levels, C = 256,
A = 3; the box head on 8 x 1000 rows of (256,7,7), hidden 1024, 22 classes; the mask head on 800 rows of (256,14,14).  Prints one JSON line.
bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 900 python bench_detheadbwd.py --out profiles/detheadbwd_bench.json

Per head: the median WALL time of `--runs` forward + backward calls (gradients to the inputs and to every parameter, synchronised before
and after), against the same layers as torch.nn modules with autograd on the device in float32 (`torch_ms`: MIOpen / rocBLAS).  No time is a
pass criterion and no ratio is fixed in advance: a head that comes out slower than torch says so (`slower_than_torch_ops`).
`wgrad_share`: the share of the weight-gradient launches (partial tiles + combine) in the device time of one forward + backward, from events.
`equal`: every layer of the head, run alone through layer_backward on a subsample (the coarsest level of image 0; 16 RoI rows; 2 mask rows)
with a seeded gradient, meets DESIGN.md section 28's single-layer bounds against float64 torch.autograd on the CPU: |dW - dW64| <= (T + 2) u
S_W, |db - db64| <= (T + 1) u S_b, |dX - dX64| <= (K + 2) u S (`largest_share_of_bound`).
Not measured: the kernels alone without the host's share; memory traffic.

    timeout -k 10 900 python bench_detheadbwd.py --train-dtype bfloat16

times DESIGN.md section 32's path instead -- DetectorHeads(trainable=True, train_dtype=torch.bfloat16): bfloat16 rows and packed weights under
float32 master weights -- at the same shapes and writes it to profiles/detheadbwd16_bench.json.  Per head, in one process, the median of
`--runs` (3) forward + backward calls after two warm-ups of: this path (`ms`), the float32 trainable heads of the same build (`float32_ms`) and
the same torch.nn modules under torch.autocast('cuda', torch.bfloat16) (`torch_ms`); `wgrad_share` from events; `kept_bytes`: the rows one
forward holds for its backward, beside `float32_kept_bytes`; `equal`: every layer alone on the subsample, fed bf16-exact operands, inside
section 32's bounds against float64 torch.autograd on the CPU.  `slower_than_float32` is the one gate: a bfloat16 head slower than the float32
head of the same process fails the run (exit status 1); `slower_than_torch_ops` is recorded, not gated."""
import argparse
import json
import statistics
import time

from bench_dethead import GRID, build_modules

U = 2.0 ** -24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--rois', type=int, default=1000, help='box head rows per frame')
    ap.add_argument('--masks', type=int, default=800, help='mask head rows')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    ap.add_argument('--train-dtype', choices=['bfloat16'], default=None, help='time DESIGN.md section 32\'s bfloat16 path instead (writes profiles/detheadbwd16_bench.json)')
    args = ap.parse_args()
    if args.train_dtype:
        return main16(args)

    import torch
    import torch.nn.functional as Fn
    from cosypose_amd import build, detector_heads as dh
    assert torch.cuda.is_available(), 'bench_detheadbwd.py needs a ROCm device'
    B, C, A, hidden, K = args.frames, args.channels, 3, 1024, 22
    R, D = B * args.rois, args.masks
    mods = build_modules(C, A, hidden, K, torch.Generator().manual_seed(args.seed))
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    rand = lambda *s: torch.randn(s, generator=gen, device='cuda')
    feats = [rand(B, C, H, W) for H, W in GRID]
    roi, mroi = rand(R, C, 7, 7), rand(D, C, 14, 14)
    heads = dh.DetectorHeads.from_modules(*mods, device='cuda', trainable=True)
    dev_mods = [type(m)() for m in mods]
    for dm, m in zip(dev_mods, mods):
        dm.load_state_dict(m.state_dict())
        dm.to(device='cuda').train().requires_grad_(True)
    t_rpn, t_box, t_pred, t_mask, t_mpred = dev_mods
    calls = {'rpn_head': (lambda x: sum(heads.rpn_head(x), []), lambda x: sum(t_rpn(x), []), feats),
             'box_head': (lambda x: list(heads.box_head(x[0])), lambda x: list(t_pred(t_box(x[0]))), [roi]),
             'mask_head': (lambda x: [heads.mask_head(x[0])], lambda x: [t_mpred(t_mask(x[0]))], [mroi])}
    params = {'rpn_head': list(t_rpn.parameters()), 'box_head': list(t_box.parameters()) + list(t_pred.parameters()),
              'mask_head': list(t_mask.parameters()) + list(t_mpred.parameters())}
    grads = {}

    def step(stage, ours):
        fwd, inputs = calls[stage][0 if ours else 1], [t.detach().requires_grad_() for t in calls[stage][2]]
        outs = fwd(inputs)
        if stage not in grads:
            grads[stage] = [torch.randn(o.shape, generator=gen, device='cuda') for o in outs]
        for p in (getattr(heads, stage).parameters() if ours else params[stage]):
            p.grad = None
        torch.autograd.backward(outs, grads[stage])
        return inputs

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

    def wgrad_share(stage):
        """device time between events around every weight-gradient call, over the device time of the whole step"""
        spans, plain = [], dh._wgrad

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = plain(*a)
            e1.record()
            spans.append((e0, e1))
            return out
        dh._wgrad = timed
        try:
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s0.record()
            step(stage, True)
            s1.record()
            torch.cuda.synchronize()
        finally:
            dh._wgrad = plain
        return round(sum(a.elapsed_time(b) for a, b in spans) / s0.elapsed_time(s1), 3)

    def layer_check(layer, x):
        """one TrainableLayer alone on the subsample x (CPU float32) -> the largest share of its three bounds"""
        g_gen = torch.Generator().manual_seed(args.seed + 1)
        ws = [w.detach().cpu().double() for w, _ in layer.pairs]
        w64 = torch.cat(ws, 1 if layer.kind == 'deconv' else 0)

        def f(xx, ww):
            if layer.kind == 'linear':
                return Fn.linear(xx, ww)
            if layer.kind == 'deconv':
                return Fn.conv_transpose2d(xx, ww, stride=2)
            return Fn.conv2d(xx, ww, padding=ww.shape[2] // 2)
        x64 = x.double()
        g = torch.randn(f(x64, w64).shape, generator=g_gen, dtype=torch.float64).float()

        def grads64(xx, ww, gg):
            xx, ww = xx.clone().requires_grad_(), ww.clone().requires_grad_()
            f(xx, ww).backward(gg)
            return xx.grad, ww.grad
        dx64, dw64 = grads64(x64, w64, g.double())
        Sx, Sw = grads64(x64.abs(), w64.abs(), g.double().abs())
        axes = [d for d in range(g.dim()) if d != 1]
        db64, Sb = g.double().sum(axes), g.double().abs().sum(axes)
        dx, got = dh.layer_backward(layer, x.cuda().contiguous(), g.cuda())
        dw = torch.cat([t.cpu().double() for t in got[0::2]], 1 if layer.kind == 'deconv' else 0)
        db = torch.cat([t.cpu().double() for t in got[1::2]])
        T = x.shape[0] * (1 if layer.kind == 'linear' else x.shape[2] * x.shape[3])
        Tb = 4 * T if layer.kind == 'deconv' else T
        Kred = w64.numel() // layer.c_in
        share = lambda got_, want, bound: float(((got_ - want).abs() / bound.clamp(min=1e-300)).max())
        return max(share(dw, dw64, (T + 2) * U * Sw), share(db, db64, (Tb + 1) * U * Sb), share(dx.cpu().double(), dx64, (Kred + 2) * U * Sx))

    def subsample_inputs(stage):
        """the input of every layer of the head on the subsample: the float32 torch chain on the CPU"""
        with torch.no_grad():
            if stage == 'rpn_head':
                x = feats[-1][:1].cpu()
                return [x, torch.relu(mods[0].conv(x))]
            if stage == 'box_head':
                x = roi[:16].flatten(1).cpu()
                h6 = torch.relu(mods[1].fc6(x))
                return [x, h6, torch.relu(mods[1].fc7(h6))]
            xs = [mroi[:2].cpu()]
            for i in range(1, 5):
                xs.append(torch.relu(getattr(mods[3], f'mask_fcn{i}')(xs[-1])))
            return xs + [torch.relu(mods[4].conv5_mask(xs[-1]))]

    layers = {'rpn_head': [heads.rpn_head.conv, heads.rpn_head.pred], 'box_head': [heads.box_head.fc6, heads.box_head.fc7, heads.box_head.pred],
              'mask_head': heads.mask_head.convs + [heads.mask_head.deconv, heads.mask_head.logits]}
    stages = {}
    for stage in ('rpn_head', 'box_head', 'mask_head'):
        share = max(layer_check(layer, x) for layer, x in zip(layers[stage], subsample_inputs(stage)))
        ms, runs = wall(lambda: step(stage, True))
        t_ms, t_runs = wall(lambda: step(stage, False))
        stages[stage] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, wgrad_share=wgrad_share(stage), equal=bool(share <= 1.0),
                             largest_share_of_bound=share, speedup_vs_torch_ops=round(t_ms / ms, 2), slower_than_torch_ops=ms > t_ms)
        torch.cuda.empty_cache()
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector heads, float32: forward + backward of the RPN head, the box head and the mask head, sum of the median wall times',
        'value': round(sum(s['ms'] for s in stages.values()), 3), 'unit': 'ms', 'higher_is_better': False,
        'torch_ms': round(sum(s['torch_ms'] for s in stages.values()), 3), 'stages': stages, 'equal': all(s['equal'] for s in stages.values()),
        'pack_count': heads.pack_count,
        'not_measured': ['kernel time without the host\'s share', '16-bit training (not built)', 'memory traffic', 'the trunk\'s backward (not built)'],
        'config': {'seed': args.seed, 'frames': B, 'levels': [list(g) for g in GRID], 'anchors_per_cell': A, 'channels': C, 'box_rows': R,
                   'hidden': hidden, 'classes': K, 'mask_rows': D, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


def main16(args):
    import torch
    import torch.nn.functional as Fn
    from cosypose_amd import build, detector_heads as dh
    assert torch.cuda.is_available(), 'bench_detheadbwd.py needs a ROCm device'
    BF16, U16, UB = torch.bfloat16, 2.0 ** -23, 2.0 ** -8
    B, C, A, hidden, K = args.frames, args.channels, 3, 1024, 22
    R, D, warmup = B * args.rois, args.masks, max(args.warmup, 2)
    mods = build_modules(C, A, hidden, K, torch.Generator().manual_seed(args.seed))
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    rand = lambda *s: torch.randn(s, generator=gen, device='cuda')
    feats = [rand(B, C, H, W) for H, W in GRID]
    roi, mroi = rand(R, C, 7, 7), rand(D, C, 14, 14)
    heads16 = dh.DetectorHeads.from_modules(*mods, device='cuda', trainable=True, train_dtype=BF16)
    heads32 = dh.DetectorHeads.from_modules(*mods, device='cuda', trainable=True)
    dev_mods = [type(m)() for m in mods]
    for dm, m in zip(dev_mods, mods):
        dm.load_state_dict(m.state_dict())
        dm.to(device='cuda').train().requires_grad_(True)
    t_rpn, t_box, t_pred, t_mask, t_mpred = dev_mods
    ours = lambda heads: {'rpn_head': lambda x: sum(heads.rpn_head(x), []), 'box_head': lambda x: list(heads.box_head(x[0])),
                          'mask_head': lambda x: [heads.mask_head(x[0])]}
    calls = {'bf16': ours(heads16), 'f32': ours(heads32),
             'torch': {'rpn_head': lambda x: sum(t_rpn(x), []), 'box_head': lambda x: list(t_pred(t_box(x[0]))), 'mask_head': lambda x: [t_mpred(t_mask(x[0]))]}}
    inputs_of = {'rpn_head': feats, 'box_head': [roi], 'mask_head': [mroi]}
    params = {'bf16': lambda st: getattr(heads16, st).parameters(), 'f32': lambda st: getattr(heads32, st).parameters(),
              'torch': lambda st: {'rpn_head': list(t_rpn.parameters()), 'box_head': list(t_box.parameters()) + list(t_pred.parameters()),
                                   'mask_head': list(t_mask.parameters()) + list(t_mpred.parameters())}[st]}
    grads = {}

    def step(stage, which):
        inputs = [t.detach().requires_grad_() for t in inputs_of[stage]]
        if which == 'torch':
            with torch.autocast('cuda', BF16):
                outs = calls[which][stage](inputs)
        else:
            outs = calls[which][stage](inputs)
        if stage not in grads:
            grads[stage] = [torch.randn(o.shape, generator=gen, device='cuda') for o in outs]
        for p in params[which](stage):
            p.grad = None
        torch.autograd.backward(outs, [g.to(o.dtype) for g, o in zip(grads[stage], outs)])
        return inputs

    def wall(call):
        for _ in range(warmup):
            call()
        out = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(out), 3), [round(v, 3) for v in out]

    def wgrad_share(stage):
        """device time between events around every weight-gradient call, over the device time of the whole step"""
        spans, plain = [], dh._wgrad

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = plain(*a)
            e1.record()
            spans.append((e0, e1))
            return out
        dh._wgrad = timed
        try:
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s0.record()
            step(stage, 'bf16')
            s1.record()
            torch.cuda.synchronize()
        finally:
            dh._wgrad = plain
        return round(sum(a.elapsed_time(b) for a, b in spans) / s0.elapsed_time(s1), 3)

    def kept_bytes(heads, stage):
        """bytes of the rows one forward of the head holds for its backward"""
        head = getattr(heads, stage)
        head.keep_rows = True
        step(stage, 'bf16' if heads is heads16 else 'f32')
        head.keep_rows = False
        k, head.last_rows = head.last_rows, None
        rows = {'rpn_head': lambda: [k['x'], k['hidden']], 'box_head': lambda: [k['x'], k['h6'], k['h7']], 'mask_head': lambda: k['rows'] + [k['up']]}[stage]()
        return int(sum(t.numel() * t.element_size() for t in rows))

    def layer_check(layer, x):
        """one TrainableLayer alone on the subsample x (CPU float32, rounded to bfloat16 here) -> the largest share of section 32's three bounds"""
        g_gen = torch.Generator().manual_seed(args.seed + 1)
        r16 = lambda t: t.to(BF16).double()
        w64 = r16(torch.cat([w.detach().cpu() for w, _ in layer.pairs], 1 if layer.kind == 'deconv' else 0))

        def f(xx, ww):
            if layer.kind == 'linear':
                return Fn.linear(xx, ww)
            if layer.kind == 'deconv':
                return Fn.conv_transpose2d(xx, ww, stride=2)
            return Fn.conv2d(xx, ww, padding=ww.shape[2] // 2)
        x64 = r16(x)
        g64 = r16(torch.randn(f(x64, w64).shape, generator=g_gen, dtype=torch.float64).float())

        def grads64(xx, ww, gg):
            xx, ww = xx.clone().requires_grad_(), ww.clone().requires_grad_()
            f(xx, ww).backward(gg)
            return xx.grad, ww.grad
        dx64, dw64 = grads64(x64, w64, g64)
        Sx, Sw = grads64(x64.abs(), w64.abs(), g64.abs())
        axes = [d for d in range(g64.dim()) if d != 1]
        db64, Sb = g64.sum(axes), g64.abs().sum(axes)
        dx, got = dh.layer_backward(layer, x64.float().cuda().contiguous(), g64.float().cuda())      # the NCHW store: float32, unrounded
        dw = torch.cat([t.cpu().double() for t in got[0::2]], 1 if layer.kind == 'deconv' else 0)
        db = torch.cat([t.cpu().double() for t in got[1::2]])
        T = x.shape[0] * (1 if layer.kind == 'linear' else x.shape[2] * x.shape[3])
        Tb = 4 * T if layer.kind == 'deconv' else T
        Kred = w64.numel() // layer.c_in
        share = lambda got_, want, bound: float(((got_ - want).abs() / bound.clamp(min=1e-300)).max())
        return max(share(dw, dw64, (T + 2) * U16 * Sw), share(db, db64, (Tb + 1) * U16 * Sb), share(dx.cpu().double(), dx64, (Kred + 2) * U16 * Sx))

    def subsample_inputs(stage):
        with torch.no_grad():
            if stage == 'rpn_head':
                x = feats[-1][:1].cpu()
                return [x, torch.relu(mods[0].conv(x))]
            if stage == 'box_head':
                x = roi[:16].flatten(1).cpu()
                h6 = torch.relu(mods[1].fc6(x))
                return [x, h6, torch.relu(mods[1].fc7(h6))]
            xs = [mroi[:2].cpu()]
            for i in range(1, 5):
                xs.append(torch.relu(getattr(mods[3], f'mask_fcn{i}')(xs[-1])))
            return xs + [torch.relu(mods[4].conv5_mask(xs[-1]))]

    layers = {'rpn_head': [heads16.rpn_head.conv, heads16.rpn_head.pred], 'box_head': [heads16.box_head.fc6, heads16.box_head.fc7, heads16.box_head.pred],
              'mask_head': heads16.mask_head.convs + [heads16.mask_head.deconv, heads16.mask_head.logits]}
    stages = {}
    for stage in ('rpn_head', 'box_head', 'mask_head'):
        share = max(layer_check(layer, x) for layer, x in zip(layers[stage], subsample_inputs(stage)))
        ms, runs = wall(lambda: step(stage, 'bf16'))
        f_ms, f_runs = wall(lambda: step(stage, 'f32'))
        t_ms, t_runs = wall(lambda: step(stage, 'torch'))
        stages[stage] = dict(ms=ms, runs_ms=runs, float32_ms=f_ms, float32_runs_ms=f_runs, torch_ms=t_ms, torch_runs_ms=t_runs, wgrad_share=wgrad_share(stage),
                             kept_bytes=kept_bytes(heads16, stage), float32_kept_bytes=kept_bytes(heads32, stage), equal=bool(share <= 1.0),
                             largest_share_of_bound=share, speedup_vs_torch_ops=round(t_ms / ms, 2), slower_than_torch_ops=ms > t_ms,
                             speedup_vs_float32=round(f_ms / ms, 2), slower_than_float32=ms > f_ms)
        torch.cuda.empty_cache()
    stamp = build.read_stamp() or {}
    total = lambda key: round(sum(s[key] for s in stages.values()), 3)
    result = {
        'metric': 'detector heads, bfloat16 rows under float32 master weights: forward + backward of the RPN head, the box head and the mask head, sum of the '
                  'median wall times',
        'value': total('ms'), 'unit': 'ms', 'higher_is_better': False, 'float32_ms': total('float32_ms'), 'torch_ms': total('torch_ms'),
        'torch': 'torch.autocast(cuda, bfloat16)', 'stages': stages, 'equal': all(s['equal'] for s in stages.values()),
        'slower_than_float32': any(s['slower_than_float32'] for s in stages.values()), 'slower_than_torch_ops': any(s['slower_than_torch_ops'] for s in stages.values()),
        'pack_count': heads16.pack_count,
        'not_measured': ['kernel time without the host\'s share', 'memory traffic', 'LDS bank conflicts of the deconvolution\'s images (predicted, no counter run)',
                         'float16 training (not built)'],
        'config': {'seed': args.seed, 'frames': B, 'levels': [list(g) for g in GRID], 'anchors_per_cell': A, 'channels': C, 'box_rows': R, 'hidden': hidden,
                   'classes': K, 'mask_rows': D, 'runs': args.runs, 'warmup': warmup, 'train_dtype': 'bfloat16'},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    with open(args.out or 'profiles/detheadbwd16_bench.json', 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))
    return 1 if result['slower_than_float32'] else 0


if __name__ == '__main__':
    raise SystemExit(main())

#!/usr/bin/env python3
"""Timing of the detector's training side (cosypose_amd.detector_train, csrc/kernels_dettrain.hip) on one GPU at the reference's training
shape: 8 frames of 480x640, five levels from 120x160 down to 8x10 with A = 3 (76 740 anchors per image), 20 ground truths per image with
masks, 22 classes, 2000 proposals per image, M = 28.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is
not affected.

    timeout -k 10 600 python bench_dettrain.py --out profiles/dettrain_bench.json

Stages, each the median WALL time of `--runs` calls after `--warmup` (device work and the host's share, synchronised before and after),
backward included where there is one: rpn_loss, roi_training_samples, fastrcnn_loss, maskrcnn_loss, and the four together.  Each is timed in
the same process against the same contract written with torch ops on the device with the same keys (`torch_ms`): box_iou as broadcast tensor
ops and max / where per image, nonzero + stable sort for the sampler, F.binary_cross_entropy_with_logits / F.l1_loss / F.cross_entropy /
F.smooth_l1_loss with autograd's backward, and for the mask targets a gather-based bilinear over groups of RoIs with the same adaptive grid.
No ratio is fixed in advance: a stage that comes out slower than the torch-ops route says so (`slower_than_torch_ops`).  `equal`: the two
routes agree on the sampled sets and labels exactly and on the losses to 2e-5 relative (both are float32 evaluations; DESIGN.md section 23
holds the kernels to float64 within derived bounds in the tests)."""
import argparse
import json
import statistics
import time

GRID = [(120, 160), (60, 80), (30, 40), (15, 20), (8, 10)]
NET = (480, 640)


# ---- the same contract in torch ops ------------------------------------------------------------------------------------------------------
def t_iou(gt, c):
    import torch
    area_g, area_c = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    wh = (torch.min(gt[:, None, 2:], c[None, :, 2:]) - torch.max(gt[:, None, :2], c[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    v = inter / (area_g[:, None] + area_c[None, :] - inter)
    return torch.where(v > 0, v, torch.zeros_like(v))


def t_match(gt, c, high, low, allow_low_quality):
    import torch
    iou = t_iou(gt, c)
    val, arg = iou.max(0)
    m = torch.where(val < low, torch.full_like(arg, -1), torch.where(val < high, torch.full_like(arg, -2), arg))
    if allow_low_quality:
        m = torch.where((iou == iou.max(1)[0][:, None]).any(0), arg, m)
    return m


def t_sample(labels, keys, bs, n_pos_max):
    import torch
    pos, neg = torch.nonzero(labels >= 1).reshape(-1), torch.nonzero(labels == 0).reshape(-1)
    n_pos = min(n_pos_max, pos.numel())
    n_neg = min(bs - n_pos, neg.numel())
    tp = pos[torch.sort(keys[pos], stable=True)[1][:n_pos]]
    tn = neg[torch.sort(keys[neg], stable=True)[1][:n_neg]]
    return torch.sort(torch.cat([tp, tn]))[0], torch.sort(tp)[0]


def t_encode(ref, p, w):
    import torch
    ew, eh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    ecx, ecy = p[:, 0] + 0.5 * ew, p[:, 1] + 0.5 * eh
    gw, gh = ref[:, 2] - ref[:, 0], ref[:, 3] - ref[:, 1]
    gcx, gcy = ref[:, 0] + 0.5 * gw, ref[:, 1] + 0.5 * gh
    return torch.stack([w[0] * (gcx - ecx) / ew, w[1] * (gcy - ecy) / eh, w[2] * torch.log(gw / ew), w[3] * torch.log(gh / eh)], 1)


def t_rpn_loss(obj, dl, gts, anchors, keys):
    import torch
    import torch.nn.functional as F
    B = obj[0].shape[0]
    logits = torch.cat([o.permute(0, 2, 3, 1).reshape(B, -1) for o in obj], 1)
    rel = torch.cat([d.view(B, -1, 4, d.shape[2], d.shape[3]).permute(0, 3, 4, 1, 2).reshape(B, -1, 4) for d in dl], 1)
    x, y, d, t, sampled = [], [], [], [], []
    for b in range(B):
        m = t_match(gts[b], anchors, 0.7, 0.3, True)
        lab = torch.where(m >= 0, torch.ones_like(m), torch.where(m == -1, torch.zeros_like(m), torch.full_like(m, -1)))
        samp, pos = t_sample(lab, keys[b], 256, 128)
        x.append(logits[b, samp]); y.append((m[samp] >= 0).float())
        d.append(rel[b, pos]); t.append(t_encode(gts[b][m[pos]], anchors[pos], (1.0, 1.0, 1.0, 1.0)))
        sampled.append(samp)
    x, y = torch.cat(x), torch.cat(y)
    return F.binary_cross_entropy_with_logits(x, y), F.l1_loss(torch.cat(d), torch.cat(t), reduction='sum') / x.numel(), sampled


def t_roi_samples(props, gts, gls, keys, bs=512, n_pos_max=128):
    import torch
    out = []
    for b, (gt, gl) in enumerate(zip(gts, gls)):
        cand = torch.cat([props[b], gt])
        m = t_match(gt, cand, 0.5, 0.5, False)
        lab = torch.where(m >= 0, gl[m.clamp(min=0)], torch.where(m == -1, torch.zeros_like(m), torch.full_like(m, -1)))
        samp, pos = t_sample(lab, keys[b, :len(cand)], bs, n_pos_max)
        cl = m.clamp(min=0)
        out.append(dict(idx=samp, boxes=cand[samp], labels=lab[samp], matched=cl[samp], targets=t_encode(gt[cl[samp]], cand[samp], (10.0, 10.0, 5.0, 5.0)),
                        pos_boxes=cand[pos], pos_labels=lab[pos], pos_matched=cl[pos]))
    return out


def t_fastrcnn_loss(z, d, labels, t):
    import torch
    import torch.nn.functional as F
    real = labels >= 0
    pos = torch.nonzero(labels > 0).reshape(-1)
    picked = d.view(d.shape[0], -1, 4)[pos, labels[pos].long()]
    return F.cross_entropy(z[real], labels[real].long()), F.smooth_l1_loss(picked, t[pos], reduction='sum') / real.sum()


def t_mask_targets(masks, boxes, matched, M):
    """roi_align with the adaptive grid over groups of RoIs that share (g_h, g_w): taps gathered from the uint8 masks"""
    import torch
    dev = boxes.device
    H, W = masks.shape[1:]
    size_w, size_h = (boxes[:, 2] - boxes[:, 0]).clamp(min=1), (boxes[:, 3] - boxes[:, 1]).clamp(min=1)
    gw, gh = torch.ceil(size_w / M).long(), torch.ceil(size_h / M).long()
    out = torch.zeros((len(boxes), M, M), dtype=torch.float32, device=dev)

    def axis(lo, size_box, g, size):
        grid = (torch.arange(M, device=dev, dtype=torch.float32)[:, None] + (torch.arange(g, device=dev, dtype=torch.float32)[None, :] + 0.5) / g).reshape(-1)
        v = lo[:, None] + grid[None, :] * (size_box / M)[:, None]
        ok = (v >= -1) & (v <= size)
        v = v.clamp(min=0)
        low = v.floor().long().clamp(max=size - 1)
        high = (low + 1).clamp(max=size - 1)
        l = torch.where(low >= size - 1, torch.zeros_like(v), v - low)
        return ok, low, high, l, 1 - l
    for g_h, g_w in torch.unique(torch.stack([gh, gw], 1), dim=0).tolist():
        r = torch.nonzero((gh == g_h) & (gw == g_w)).reshape(-1)
        oy, y0, y1, ly, hy = axis(boxes[r, 1], size_h[r], g_h, H)
        ox, x0, x1, lx, hx = axis(boxes[r, 0], size_w[r], g_w, W)
        tap = lambda yy, xx: masks[matched[r].long()[:, None, None], yy[:, :, None], xx[:, None, :]].float()
        wgt = lambda a, b: a[:, :, None] * b[:, None, :]
        v = wgt(hy, hx) * tap(y0, x0) + wgt(hy, lx) * tap(y0, x1) + wgt(ly, hx) * tap(y1, x0) + wgt(ly, lx) * tap(y1, x1)
        v = v * (oy[:, :, None] & ox[:, None, :])
        out[r] = v.reshape(len(r), M, g_h, M, g_w).sum((2, 4)) / (g_h * g_w)
    return out


def t_mask_loss(x, boxes, labels, matched, masks, counts, rows):
    import torch
    import torch.nn.functional as F
    M = x.shape[-1]
    picked, targets = [], []
    for b, n in enumerate(counts):
        r = slice(b * rows, b * rows + n)
        targets.append(t_mask_targets(masks[b], boxes[r], matched[r], M))
        picked.append(x[r][torch.arange(n, device=x.device), labels[r].long()])
    return F.binary_cross_entropy_with_logits(torch.cat(picked), torch.cat(targets))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd import detector_train as dt
    from cosypose_amd.detector_rpn import rpn_anchors
    assert torch.cuda.is_available(), 'bench_dettrain.py needs a ROCm device'
    B, A, G, C, post, M, bs, n_pos_max = args.frames, 3, 20, 22, 2000, 28, 512, 128
    rng = np.random.RandomState(args.seed)
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    obj = [torch.randn((B, A, H, W), generator=gen, device='cuda') for H, W in GRID]
    dl = [torch.randn((B, 4 * A, H, W), generator=gen, device='cuda') * 0.2 for H, W in GRID]
    gts, gls, masks, props = [], [], [], []
    for b in range(B):
        w, h = rng.uniform(40, 200, G), rng.uniform(40, 200, G)
        x1, y1 = rng.uniform(0, NET[1] - w), rng.uniform(0, NET[0] - h)
        gt = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
        mk = np.zeros((G,) + NET, np.uint8)
        for g, (a, c, e, f) in enumerate(gt.astype(int)):
            mk[g, c:f, a:e] = 1
        near = gt[rng.randint(0, G, post // 2)] + rng.normal(0, 8, (post // 2, 4)).astype(np.float32)       # half the proposals near a ground truth
        px, py = rng.uniform(0, NET[1] - 20, post - post // 2), rng.uniform(0, NET[0] - 20, post - post // 2)
        far = np.stack([px, py, px + rng.uniform(10, 300, len(px)), py + rng.uniform(10, 300, len(px))], 1).astype(np.float32)
        p = np.concatenate([near, far])[rng.permutation(post)]
        p[:, [0, 2]], p[:, [1, 3]] = np.sort(p[:, [0, 2]].clip(0, NET[1]), 1), np.sort(p[:, [1, 3]].clip(0, NET[0]), 1)
        p[:, 2:] = np.maximum(p[:, 2:], p[:, :2] + 1)
        gts.append(cuda(gt)); gls.append(cuda(rng.randint(1, C, G))); masks.append(cuda(mk)); props.append(cuda(p))
    targets = [dict(boxes=g, labels=l, masks=m) for g, l, m in zip(gts, gls, masks)]
    gls32 = [l.to(torch.int32) for l in gls]
    proposals, counts = torch.cat(props), torch.full((B,), post, dtype=torch.int32, device='cuda')
    props3 = torch.stack(props)
    nets = [NET] * B
    anchors = rpn_anchors(GRID, NET).cuda()
    N = anchors.shape[0]
    keys_rpn = torch.randint(0, 2 ** 31 - 1, (B, N), dtype=torch.int32, device='cuda', generator=gen)
    keys_roi = torch.randint(0, 2 ** 31 - 1, (B, post + G), dtype=torch.int32, device='cuda', generator=gen)
    class_logits = torch.randn((B * bs, C), generator=gen, device='cuda') * 2
    box_regression = torch.randn((B * bs, 4 * C), generator=gen, device='cuda')
    mask_logits = torch.randn((B * n_pos_max, C, M, M), generator=gen, device='cuda')

    def leaves(*ts):
        return [t.detach().clone().requires_grad_() for t in ts]

    # ---- our route -----------------------------------------------------------------------------------------------------------------------
    def ours_rpn():
        heads = leaves(*obj, *dl)
        l1, l2 = dt.rpn_loss(heads[:5], heads[5:], targets, nets, NET, keys=keys_rpn)
        (l1 + l2).backward()
        return l1, l2

    def ours_roi():
        return dt.roi_training_samples(proposals, counts, targets, keys=keys_roi)
    smp = ours_roi()

    def ours_frc():
        z, d = leaves(class_logits, box_regression)
        l1, l2 = dt.fastrcnn_loss(z, d, smp['labels'], smp['regression_targets'])
        (l1 + l2).backward()
        return l1, l2

    def ours_mask(s=smp):
        x, = leaves(mask_logits)
        loss = dt.maskrcnn_loss(x, s['pos_boxes'], s['pos_labels'], s['pos_matched_idxs'], targets, s['pos_counts'])
        loss.backward()
        return loss

    def ours_all():
        a = ours_rpn()
        s = ours_roi()
        z, d = leaves(class_logits, box_regression)
        l1, l2 = dt.fastrcnn_loss(z, d, s['labels'], s['regression_targets'])
        (l1 + l2).backward()
        return a + (l1, l2, ours_mask(s))

    # ---- the torch-ops route ----------------------------------------------------------------------------------------------------------------
    def torch_rpn():
        heads = leaves(*obj, *dl)
        l1, l2, sampled = t_rpn_loss(heads[:5], heads[5:], gts, anchors, keys_rpn)
        (l1 + l2).backward()
        return l1, l2, sampled

    def torch_roi():
        return t_roi_samples(props3, gts, gls32, keys_roi)
    t_smp = torch_roi()

    def pad_rows(parts, rows, fill):
        out = torch.full((B * rows,) + tuple(parts[0].shape[1:]), fill, dtype=parts[0].dtype, device='cuda')
        for b, p in enumerate(parts):
            out[b * rows:b * rows + len(p)] = p
        return out

    def torch_frc(s=None):
        s = s or t_smp
        z, d = leaves(class_logits, box_regression)
        labels, t = pad_rows([q['labels'] for q in s], bs, -1), pad_rows([q['targets'] for q in s], bs, 0.0)
        l1, l2 = t_fastrcnn_loss(z, d, labels, t)
        (l1 + l2).backward()
        return l1, l2

    def torch_mask(s=None):
        s = s or t_smp
        x, = leaves(mask_logits)
        n = [len(q['pos_boxes']) for q in s]
        loss = t_mask_loss(x, pad_rows([q['pos_boxes'] for q in s], n_pos_max, 0.0), pad_rows([q['pos_labels'] for q in s], n_pos_max, 0),
                           pad_rows([q['pos_matched'] for q in s], n_pos_max, 0), masks, n, n_pos_max)
        loss.backward()
        return loss

    def torch_all():
        a = torch_rpn()[:2]
        s = torch_roi()
        return a + torch_frc(s) + (torch_mask(s),)

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

    # ---- agreement ---------------------------------------------------------------------------------------------------------------------------
    close = lambda a, b: abs(a.item() - b.item()) <= 2e-5 * max(1.0, abs(b.item()))
    o_rpn = dt.rpn_loss(obj, dl, targets, nets, NET, keys=keys_rpn, return_samples=True)
    t_rpn = torch_rpn()
    same_rpn = all(o_rpn[2][1][b, :int(o_rpn[2][2][b])].tolist() == t_rpn[2][b].tolist() for b in range(B))
    n_roi, n_pos = smp['counts'].tolist(), smp['pos_counts'].tolist()
    same_roi = all(n_roi[b] == len(q['idx']) and n_pos[b] == len(q['pos_boxes']) and torch.equal(smp['labels'][b * bs:b * bs + n_roi[b]], q['labels'])
                   and torch.equal(smp['boxes'][b * bs:b * bs + n_roi[b]], q['boxes']) and torch.equal(smp['pos_matched_idxs'][b * n_pos_max:b * n_pos_max + n_pos[b]], q['pos_matched'].to(torch.int32))
                   for b, q in enumerate(t_smp))
    o_frc, t_frc, o_mask, t_mask = ours_frc(), torch_frc(), ours_mask(), torch_mask()
    pairs = dict(loss_objectness=(o_rpn[0], t_rpn[0]), loss_rpn_box_reg=(o_rpn[1], t_rpn[1]), loss_classifier=(o_frc[0], t_frc[0]),
                 loss_box_reg=(o_frc[1], t_frc[1]), loss_mask=(o_mask, t_mask))
    losses = {k: dict(ours=a.item(), torch_ops=b.item(), close=close(a, b)) for k, (a, b) in pairs.items()}

    stages = {}
    for name, ours, ref_call, equal in (('rpn_loss', ours_rpn, torch_rpn, same_rpn and losses['loss_objectness']['close'] and losses['loss_rpn_box_reg']['close']),
                                        ('roi_training_samples', ours_roi, torch_roi, same_roi),
                                        ('fastrcnn_loss', ours_frc, torch_frc, losses['loss_classifier']['close'] and losses['loss_box_reg']['close']),
                                        ('maskrcnn_loss', ours_mask, torch_mask, losses['loss_mask']['close']),
                                        ('all_four', ours_all, torch_all, None)):
        ms, runs = wall(ours, args.runs, args.warmup)
        t_ms, t_runs = wall(ref_call, args.runs, args.warmup)
        stages[name] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, speedup_vs_torch_ops=round(t_ms / ms, 2), slower_than_torch_ops=ms > t_ms)
        if equal is not None:
            stages[name]['equal'] = bool(equal)
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector training side: rpn_loss + roi_training_samples + fastrcnn_loss + maskrcnn_loss with backward, median wall time of the four together',
        'value': stages['all_four']['ms'], 'unit': 'ms', 'higher_is_better': False, 'torch_ms': stages['all_four']['torch_ms'],
        'stages': stages, 'losses': losses, 'equal': all(s.get('equal', True) for s in stages.values()),
        'sampled': {'rpn_per_frame': o_rpn[2][2].tolist(), 'roi_per_frame': n_roi, 'positives_per_frame': n_pos},
        'config': {'seed': args.seed, 'frames': B, 'net': list(NET), 'levels': [list(g) for g in GRID], 'anchors_per_cell': A, 'anchors_per_frame': int(N),
                   'ground_truths_per_frame': G, 'classes': C, 'proposals_per_frame': post, 'mask_side': M, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

"""The twin of the detector's proposal side: torchvision 0.4.2's AnchorGenerator, RegionProposalNetwork.
filter_proposals and MultiScaleRoIAlign with Mask R-CNN's defaults, restated from the contract's text over float32 CPU operations.  It imports
nothing from cosypose_amd and reads nothing outside tests/; NMS comes from detpost_ref.py (the twin of section 21).  torchvision itself is not
installed where this was written: the twin has never been run against it.

Selection: a stable descending argsort in float32 after the NaN anchors are removed.  Decode: float32 torch CPU operations.  RoIAlign: the
stated operation order in NumPy float32, one rounding per operation (the loops over the g x g samples are explicit, the P x P bins and the
channels are array axes: every element sees the same scalar operations in the same order).  roi_align64: the same samples with weights, products
and sums in float64, and sum |w p| for the error bound."""
import math

import numpy as np
import torch

import detpost_ref as post

XFORM_CLIP = math.log(1000.0 / 16)
DEFAULT_SIZES = ((32,), (64,), (128,), (256,), (512,))
DEFAULT_RATIOS = (0.5, 1.0, 2.0)
F = np.float32


# ---- anchors -----------------------------------------------------------------------------------------------------------------------
def base_anchors(sizes, aspect_ratios=DEFAULT_RATIOS):
    scales, ar = torch.tensor(sizes, dtype=torch.float32).reshape(-1), torch.tensor(aspect_ratios, dtype=torch.float32)
    h_r = torch.sqrt(ar)
    w_r = 1 / h_r
    ws, hs = (w_r[:, None] * scales[None, :]).reshape(-1), (h_r[:, None] * scales[None, :]).reshape(-1)
    return (torch.stack([-ws, -hs, ws, hs], 1) / 2).round().numpy()          # torch rounds half to even


def level_anchors(H, W, padded_size, sizes, aspect_ratios=DEFAULT_RATIOS):
    """(H W A, 4): row (y W + x) A + a"""
    base = torch.from_numpy(base_anchors(sizes, aspect_ratios))
    stride_h, stride_w = torch.tensor(padded_size[0] / H, dtype=torch.float32), torch.tensor(padded_size[1] / W, dtype=torch.float32)
    sx, sy = torch.arange(W, dtype=torch.float32) * stride_w, torch.arange(H, dtype=torch.float32) * stride_h
    yy, xx = torch.meshgrid(sy, sx, indexing='ij')
    shift = torch.stack([xx, yy, xx, yy], -1).reshape(-1, 1, 4)
    return (shift + base[None]).reshape(-1, 4).numpy()


def anchors(feature_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS):
    return np.concatenate([level_anchors(H, W, padded_size, s, aspect_ratios) for (H, W), s in zip(feature_sizes, sizes)])


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def flatten_level(objectness, deltas):
    """one image: objectness (A,H,W), deltas (4A,H,W) -> logits (H W A), deltas (H W A, 4): torchvision's permute_and_flatten"""
    A, H, W = objectness.shape
    return (np.ascontiguousarray(objectness.transpose(1, 2, 0)).reshape(-1),
            np.ascontiguousarray(deltas.reshape(A, 4, H, W).transpose(2, 3, 0, 1)).reshape(-1, 4))


def top_k(logits, deltas, k):
    """indices of the min(k, present) largest logits by descending value, equal values lower index first; NaN anchors are absent"""
    present = np.flatnonzero(~np.isnan(logits) & ~np.isnan(deltas).any(1))
    vals = logits[present].astype(F) + F(0)                                   # -0 counts as +0
    order = np.argsort(-vals, kind='stable')[:k]
    return present[order]


def select(objectness, deltas, b, pre_nms_top_n):
    """-> per level the selected anchor indices of image b, in the twin's order"""
    return [top_k(*flatten_level(np.asarray(o[b], F), np.asarray(d[b], F)), pre_nms_top_n) for o, d in zip(objectness, deltas)]


# ---- decode ------------------------------------------------------------------------------------------------------------------------
def decode(deltas, boxes):
    """BoxCoder.decode_single with weights (1,1,1,1): (N,4), (N,4) -> (N,4); section 21 step 2's operation sequence with weight 1"""
    rel, p = post.f32(deltas).reshape(-1, 4), post.f32(boxes).reshape(-1, 4)
    w, h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    cx, cy = p[:, 0] + 0.5 * w, p[:, 1] + 0.5 * h
    dx, dy = rel[:, 0], rel[:, 1]
    dw, dh = torch.clamp(rel[:, 2], max=XFORM_CLIP), torch.clamp(rel[:, 3], max=XFORM_CLIP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)


# ---- filter_proposals --------------------------------------------------------------------------------------------------------------
def proposals(objectness, deltas, net_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS, pre_nms_top_n=1000,
              post_nms_top_n=1000, nms_thresh=0.7, min_size=1e-3):
    """lists of (B,A,H,W) / (B,4A,H,W) arrays -> one dict per image: boxes (n,4), scores, levels, src (candidate index), by descending logit,
    and `candidates`: src of what entered NMS"""
    B = objectness[0].shape[0]
    out = []
    for b in range(B):
        boxes, scores, levels, src, first = [], [], [], [], 0
        for l, (o, d) in enumerate(zip(objectness, deltas)):
            A, H, W = o.shape[1:]
            logits, rel = flatten_level(np.asarray(o[b], F), np.asarray(d[b], F))
            idx = top_k(logits, rel, pre_nms_top_n)
            anc = level_anchors(H, W, padded_size, sizes[l], aspect_ratios)
            with np.errstate(all='ignore'):
                bx = post.clip(decode(rel[idx], anc[idx]), net_sizes[b])
            boxes.append(bx); scores.append(logits[idx] + F(0)); levels.append(np.full(len(idx), l)); src.append(first + idx)
            first += A * H * W
        boxes, scores, levels, src = torch.cat(boxes), np.concatenate(scores), np.concatenate(levels), np.concatenate(src)
        big = torch.nonzero(((boxes[:, 2] - boxes[:, 0]) >= F(min_size)) & ((boxes[:, 3] - boxes[:, 1]) >= F(min_size))).reshape(-1).numpy()
        boxes, scores, levels, src = boxes[big].numpy().reshape(-1, 4), scores[big], levels[big], src[big]
        by_src = np.argsort(src, kind='stable')                               # position = candidate index order: nms visits equal scores that way
        boxes, scores, levels, src = boxes[by_src], scores[by_src], levels[by_src], src[by_src]
        keep = post.batched_nms_fast(boxes, scores, levels, nms_thresh, post_nms_top_n)
        out.append(dict(boxes=boxes[keep].reshape(-1, 4), scores=scores[keep], levels=levels[keep], src=src[keep], candidates=src))
    return out


# ---- level mapper ------------------------------------------------------------------------------------------------------------------
def level_value64(boxes):
    """4 + log2(sqrt(area) / 224 + 1e-6) in float64 (NaN for a negative area): how far a box sits from a level boundary"""
    b = np.asarray(boxes, F).astype(np.float64).reshape(-1, 4)
    with np.errstate(all='ignore'):
        return 4 + np.log2(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224 + 1e-6)


def map_levels(boxes, k_min, k_max):
    """LevelMapper in float32 -> level index (N) int; a NaN (negative area) takes level 0"""
    b = np.asarray(boxes, F).reshape(-1, 4)
    with np.errstate(all='ignore'):
        s = np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
        t = np.floor(F(4) + np.log2(s / F(224) + F(1e-6)))
    t = np.where(np.isnan(t), k_min, np.clip(t, k_min, k_max))
    return t.astype(np.int64) - k_min


def infer_scales(feature_sizes, net_sizes):
    max_h, max_w = max(s[0] for s in net_sizes), max(s[1] for s in net_sizes)
    scales = []
    for H, W in feature_sizes:
        s_h = 2.0 ** float(torch.tensor(float(H) / float(max_h)).log2().round())
        s_w = 2.0 ** float(torch.tensor(float(W) / float(max_w)).log2().round())
        assert s_h == s_w
        scales.append(s_h)
    return scales


# ---- roi_align ---------------------------------------------------------------------------------------------------------------------
def axis_taps(lo, hi, scale, P, g, size):
    """one axis of roi_align in float32 -> per (p, i): valid, low index, high index, weight of the high tap (l), of the low tap (h)"""
    with np.errstate(all='ignore'):
        start, end = F(lo) * F(scale), F(hi) * F(scale)
        ext = end - start
        extent = ext if ext > F(1) else F(1)                                  # max(extent, 1); NaN -> 1
        bin_ = extent / F(P)
        valid, il, ih, wl, wh = (np.zeros((P, g), t) for t in (bool, np.int64, np.int64, F, F))
        for p in range(P):
            for i in range(g):
                v = (start + F(p) * bin_) + ((F(i) + F(.5)) * bin_) / F(g)
                if not (v >= F(-1) and v <= F(size)):
                    continue
                if v <= 0:
                    v = F(0)
                low = int(v)
                if low >= size - 1:
                    high = low = size - 1
                    v = F(low)
                else:
                    high = low + 1
                l = v - F(low)
                valid[p, i], il[p, i], ih[p, i], wl[p, i], wh[p, i] = True, low, high, l, F(1) - l
    return valid, il, ih, wl, wh


def roi_align(feat, box, scale, P, g, dtype=F):
    """feat (C,H,W) float32, box (4) -> (C,P,P): iy outer, ix inner, each sample w1 p1 + w2 p2 + w3 p3 + w4 p4 left to right, the sum
    divided by g^2; dtype = float64 evaluates weights (from the float32 sample position), products and sums in float64 and also returns
    sum |w p| / g^2"""
    feat = np.asarray(feat, F)
    C, H, W = feat.shape
    vy, yl, yh, ly, hy = axis_taps(box[1], box[3], scale, P, g, H)
    vx, xl, xh, lx, hx = axis_taps(box[0], box[2], scale, P, g, W)
    if dtype is not F:
        feat = feat.astype(dtype)
        ly, lx = ly.astype(dtype), lx.astype(dtype)
        hy, hx = 1 - ly, 1 - lx
    acc, mag = np.zeros((C, P, P), dtype), np.zeros((C, P, P), dtype)
    for iy in range(g):
        for ix in range(g):
            ok = vy[:, iy][:, None] & vx[:, ix][None, :]
            Y0, Y1, X0, X1 = yl[:, iy][:, None], yh[:, iy][:, None], xl[:, ix][None, :], xh[:, ix][None, :]
            HY, LY, HX, LX = hy[:, iy][:, None], ly[:, iy][:, None], hx[:, ix][None, :], lx[:, ix][None, :]
            w1, w2, w3, w4 = HY * HX, HY * LX, LY * HX, LY * LX
            t1, t2, t3, t4 = w1 * feat[:, Y0, X0], w2 * feat[:, Y0, X1], w3 * feat[:, Y1, X0], w4 * feat[:, Y1, X1]
            v = ((t1 + t2) + t3) + t4
            acc = np.where(ok[None], acc + v, acc)
            mag = np.where(ok[None], mag + (np.abs(t1) + np.abs(t2) + np.abs(t3) + np.abs(t4)), mag)
    count = dtype(g * g)
    return (acc / count) if dtype is F else (acc / count, mag / count)


def multiscale_roi_align(features, boxes, im_ids, scales, P, g, dtype=F):
    """features[l] (B,C,H_l,W_l), boxes (R,4), im_ids (R) -> (R,C,P,P), levels (R)[, magnitudes with float64]"""
    k_min, k_max = int(round(-math.log2(scales[0]))), int(round(-math.log2(scales[-1])))
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    levels = map_levels(boxes, k_min, k_max)
    C = features[0].shape[1]
    out = [roi_align(features[l][b], box, scales[l], P, g, dtype) for box, b, l in zip(boxes, im_ids, levels)]
    if dtype is F:
        return np.stack(out).reshape(-1, C, P, P) if out else np.zeros((0, C, P, P), F), levels
    vals = np.stack([o[0] for o in out]) if out else np.zeros((0, C, P, P))
    mags = np.stack([o[1] for o in out]) if out else np.zeros((0, C, P, P))
    return vals, levels, mags


# ---- features -> detections ----------------------------------------------------------------------------------------------------------
def chain(features, rpn_head, box_head, mask_head, net_sizes, padded_size, original_sizes, category_id_to_label, n_roi_levels=4, detection_th=None,
          one_instance_per_class=False, output_masks=False, mask_th=0.8, rpn_options=None, head_options=None):
    """the twin chain: numpy features; the heads are callables over numpy arrays (the test wraps the torch modules).  -> get_detections'
    dict, the per-image proposals and post-processing results"""
    objectness, deltas = rpn_head(features)
    props = proposals(objectness, deltas, net_sizes, padded_size, **(rpn_options or {}))
    roi_maps = features[:n_roi_levels]
    scales = infer_scales([f.shape[2:] for f in roi_maps], net_sizes)
    boxes = np.concatenate([p['boxes'] for p in props]).reshape(-1, 4)
    im_ids = np.concatenate([np.full(len(p['boxes']), b) for b, p in enumerate(props)]).astype(np.int64)
    class_logits, box_regression = box_head(multiscale_roi_align(roi_maps, boxes, im_ids, scales, 7, 2)[0])
    per_image = post.postprocess(class_logits, box_regression, [p['boxes'] for p in props], net_sizes, original_sizes, **(head_options or {}))

    def masks_of(boxes_net, batch_im_id):
        return mask_head(multiscale_roi_align(roi_maps, boxes_net, batch_im_id, scales, 14, 2)[0])
    res = post.get_detections(per_image, category_id_to_label, masks_of, tuple(original_sizes[0]), detection_th, one_instance_per_class, output_masks,
                              mask_th)
    return res, props, per_image

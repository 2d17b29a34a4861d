"""The twin of the detector's output side: torchvision 0.4.2's post-processing with Mask R-CNN defaults and
Detector.get_detections' filters, restated over torch CPU float32 ops -- softmax, exp, clamp, F.interpolate(bilinear,
align_corners=False) -- and a plain Python greedy NMS.  Written from the contract's text, independently of the product: it imports
nothing from cosypose_amd and reads nothing outside tests/.  torchvision itself is not installed where this was written: the twin has
never been run against it.

float64 variants of the scores (scores64) and of the pasted mask values (paste_values(..., dtype=torch.float64)) exist only to tell
near-ties: a score next to score_thresh, a mask value next to mask_th."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (10.0, 10.0, 5.0, 5.0)
XFORM_CLIP = math.log(1000.0 / 16)
MIN_SIZE = 1e-2


def f32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


# ---- steps 1-3 ---------------------------------------------------------------------------------------------------------------------
def scores32(class_logits):
    return F.softmax(f32(class_logits), -1)


def scores64(class_logits):
    return F.softmax(f32(class_logits).double(), -1)


def decode(box_regression, proposals):
    """(R,4C), (R,4) -> (R,C,4), one float32 rounding per operation"""
    rel, p = f32(box_regression), f32(proposals)
    rel = rel.reshape(p.shape[0], -1, 4)
    w, h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    cx, cy = p[:, 0] + 0.5 * w, p[:, 1] + 0.5 * h
    dx, dy = rel[:, :, 0] / WEIGHTS[0], rel[:, :, 1] / WEIGHTS[1]
    dw = torch.clamp(rel[:, :, 2] / WEIGHTS[2], max=XFORM_CLIP)
    dh = torch.clamp(rel[:, :, 3] / WEIGHTS[3], max=XFORM_CLIP)
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)


def clip(boxes, net_size):
    net_h, net_w = net_size
    out = boxes.clone()
    out[..., 0::2] = out[..., 0::2].clamp(min=0, max=net_w)
    out[..., 1::2] = out[..., 1::2].clamp(min=0, max=net_h)
    return out


# ---- step 5 ------------------------------------------------------------------------------------------------------------------------
def iou(a, b):
    """box_iou's float32 arithmetic for one pair of (4) tensors"""
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    w = (torch.min(a[2], b[2]) - torch.max(a[0], b[0])).clamp(min=0)
    h = (torch.min(a[3], b[3]) - torch.max(a[1], b[1])).clamp(min=0)
    inter = w * h
    return inter / ((area_a + area_b) - inter)


def visiting_order(scores):
    """descending score, equal scores lower index first"""
    s = np.asarray(scores, dtype=np.float32)
    return sorted(range(len(s)), key=lambda i: (-float(s[i]), i))


def iou_many(kept, b):
    """iou of every row of kept (K,4) with the box b (4): the same operations, one float32 rounding each"""
    area_k, area_b = (kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1]), (b[2] - b[0]) * (b[3] - b[1])
    w = (torch.min(kept[:, 2], b[2]) - torch.max(kept[:, 0], b[0])).clamp(min=0)
    h = (torch.min(kept[:, 3], b[3]) - torch.max(kept[:, 1], b[1])).clamp(min=0)
    inter = w * h
    return inter / ((area_k + area_b) - inter)


def nms(boxes, scores, iou_threshold, max_keep=None):
    boxes = f32(boxes).reshape(-1, 4)
    thr = torch.tensor(iou_threshold, dtype=torch.float32)
    keep = []
    for i in visiting_order(scores):
        if max_keep is not None and len(keep) >= max_keep:
            break
        if not keep or not bool((iou_many(boxes[keep], boxes[i]) > thr).any()):
            keep.append(i)
    return np.asarray(keep, dtype=np.int64)


def batched_nms(boxes, scores, idxs, iou_threshold, max_keep=None):
    boxes = f32(boxes).reshape(-1, 4)
    if boxes.numel() == 0:
        return np.zeros(0, np.int64)
    offsets = torch.as_tensor(np.asarray(idxs)).to(boxes) * (boxes.max() + 1)
    return nms(boxes + offsets[:, None], scores, iou_threshold, max_keep)


# ---- steps 1-6 of one batch ----------------------------------------------------------------------------------------------------------
def postprocess(class_logits, box_regression, proposals, net_sizes, original_sizes=None, score_thresh=0.05, nms_thresh=0.5,
                detections_per_img=100):
    """proposals: list of (R_i,4) -> one dict per image: boxes_net, boxes (frame), scores, labels (category ids), proposal (row in the
    image's proposals), all numpy, by descending score"""
    out, first = [], 0
    logits, reg = np.asarray(class_logits, np.float32), np.asarray(box_regression, np.float32)
    for b, props in enumerate(proposals):
        R = len(props)
        C = logits.shape[1]
        sc = scores32(logits[first:first + R])
        bx = clip(decode(reg[first:first + R], props), net_sizes[b])
        first += R
        label = torch.arange(C).expand(R, C)
        prop = torch.arange(R)[:, None].expand(R, C)
        bx, sc, label, prop = bx[:, 1:].reshape(-1, 4), sc[:, 1:].reshape(-1), label[:, 1:].reshape(-1), prop[:, 1:].reshape(-1)
        cand = torch.nonzero(sc > score_thresh).reshape(-1)
        bx, sc, label, prop = bx[cand], sc[cand], label[cand], prop[cand]
        big = torch.nonzero(((bx[:, 2] - bx[:, 0]) >= MIN_SIZE) & ((bx[:, 3] - bx[:, 1]) >= MIN_SIZE)).reshape(-1)
        bx, sc, label, prop = bx[big], sc[big], label[big], prop[big]
        keep = torch.as_tensor(batched_nms(bx, sc, label, nms_thresh, detections_per_img), dtype=torch.int64)
        bx, sc, label, prop = bx[keep], sc[keep], label[keep], prop[keep]
        frame = bx.clone()
        if original_sizes is not None:
            ratio_h = torch.tensor(original_sizes[b][0], dtype=torch.float32) / torch.tensor(net_sizes[b][0], dtype=torch.float32)
            ratio_w = torch.tensor(original_sizes[b][1], dtype=torch.float32) / torch.tensor(net_sizes[b][1], dtype=torch.float32)
            frame = torch.stack([bx[:, 0] * ratio_w, bx[:, 1] * ratio_h, bx[:, 2] * ratio_w, bx[:, 3] * ratio_h], 1)
        out.append(dict(boxes_net=bx.numpy().reshape(-1, 4), boxes=frame.numpy().reshape(-1, 4), scores=sc.numpy(), labels=label.numpy(),
                        proposal=prop.numpy()))
    return out


# ---- step 8 ------------------------------------------------------------------------------------------------------------------------
def box_pixels(box, M):
    """the expanded box truncated toward zero -> (bx1, by1, bx2, by2) Python ints"""
    b = f32(box)
    scale = torch.tensor(M + 2, dtype=torch.float32) / torch.tensor(M, dtype=torch.float32)
    xc, yc = (b[2] + b[0]) * 0.5, (b[3] + b[1]) * 0.5
    wh, hh = (b[2] - b[0]) * 0.5 * scale, (b[3] - b[1]) * 0.5 * scale
    return tuple(int(v) for v in torch.stack([xc - wh, yc - hh, xc + wh, yc + hh]).to(torch.int64))


def paste_values(mask_logits, boxes, labels, frame_size, dtype=torch.float32):
    """-> (D,H,W) pasted probabilities (0 outside the box) and (D,H,W) bool `inside` (pixels that took an interpolated value)"""
    H, W = frame_size
    logits = f32(mask_logits)
    D, _, M, _ = logits.shape
    values, inside = torch.zeros((D, H, W), dtype=dtype), torch.zeros((D, H, W), dtype=torch.bool)
    for d in range(D):
        prob = torch.sigmoid(logits[d, int(labels[d])].to(dtype))
        padded = F.pad(prob, (1, 1, 1, 1))
        bx1, by1, bx2, by2 = box_pixels(boxes[d], M)
        w, h = max(bx2 - bx1 + 1, 1), max(by2 - by1 + 1, 1)
        x0, x1, y0, y1 = max(bx1, 0), min(bx2 + 1, W), max(by1, 0), min(by2 + 1, H)
        if x0 >= x1 or y0 >= y1:
            continue
        if h * w <= 1 << 22:
            up = F.interpolate(padded[None, None], size=(h, w), mode='bilinear', align_corners=False)[0, 0]
            values[d, y0:y1, x0:x1] = up[y0 - by1:y1 - by1, x0 - bx1:x1 - bx1]
        else:
            raise ValueError('box too large for the twin')
        inside[d, y0:y1, x0:x1] = True
    return values, inside


def paste_masks(mask_logits, boxes, labels, frame_size, mask_th=0.8):
    return (paste_values(mask_logits, boxes, labels, frame_size)[0] > mask_th).numpy()


# ---- steps 7-8: Detector.get_detections ------------------------------------------------------------------------------------------------
def get_detections(per_image, category_id_to_label, mask_head=None, frame_size=None, detection_th=None, one_instance_per_class=False,
                   output_masks=False, mask_th=0.8):
    """per_image: postprocess' dicts -> dict(batch_im_id, label, score, bboxes[, masks], rows): the filters first (a Python loop over the
    detections, as the reference's), then the masks of the survivors only (mask_head(boxes_net, batch_im_id) -> (D,C,M,M) numpy)"""
    rows = []
    for b, out in enumerate(per_image):
        for j in range(len(out['scores'])):
            score = float(out['scores'][j])
            if detection_th is None or score > detection_th:
                rows.append((b, j, category_id_to_label[int(out['labels'][j])], score))
    if one_instance_per_class:
        best = {}
        for r in rows:                                      # the first best of every label: an earlier row wins a tie
            if r[2] not in best or r[3] > best[r[2]][3]:
                best[r[2]] = r
        order = {id(r): n for n, r in enumerate(rows)}
        rows = sorted(best.values(), key=lambda r: (-r[3], order[id(r)]))
    res = dict(batch_im_id=np.array([r[0] for r in rows], np.int64), label=np.array([str(r[2]) for r in rows], dtype=object),
               score=np.array([r[3] for r in rows], np.float64), rows=[(r[0], r[1]) for r in rows],
               bboxes=np.array([per_image[b]['boxes'][j] for b, j, _, _ in rows], np.float32).reshape(-1, 4))
    if output_masks:
        boxes_net = np.array([per_image[b]['boxes_net'][j] for b, j, _, _ in rows], np.float32).reshape(-1, 4)
        labels = np.array([per_image[b]['labels'][j] for b, j, _, _ in rows], np.int64)
        if len(rows):
            logits = mask_head(boxes_net, res['batch_im_id'])
            res['masks'] = paste_masks(logits, res['bboxes'], labels, frame_size, mask_th)
        else:
            res['masks'] = np.zeros((0,) + tuple(frame_size), bool)
    return res


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
def smooth_mask_logits(seed, D, C, M, amplitude=6.0):
    """low-frequency logits: a few pixels only come near a threshold, none sits on a plateau at it"""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, M), np.linspace(-1, 1, M), indexing='ij')
    out = np.zeros((D, C, M, M), np.float32)
    for d in range(D):
        for c in range(C):
            cx, cy, r = rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.45, 0.8)
            tilt = rng.uniform(-0.7, 0.7, 2)
            out[d, c] = amplitude * (1 - ((x - cx) ** 2 + (y - cy) ** 2) / r ** 2) + tilt[0] * x + tilt[1] * y + 0.37
    return out


def head_case(seed, counts, C, net_size, near_thresh=0.05):
    """class_logits in [-8, 8], box_regression, proposals for images of `counts` proposals; the edge cases of DESIGN section 21's test
    plan are planted in image 0: proposal 0 decodes through the log(1000/16) clamp, the last proposal of image 0 lies right of the
    image (zero width after the clip) with a high score, and (with at least 2 proposals) proposal 1 scores near_thresh + 5e-4"""
    rng = np.random.RandomState(seed)
    net_h, net_w = net_size
    R = int(sum(counts))
    logits = rng.uniform(-8, 8, (R, C)).astype(np.float32)
    reg = (rng.uniform(-1, 1, (R, C, 4)) * np.array([2, 2, 3, 3])).astype(np.float32)
    x1, y1 = rng.uniform(0, net_w - 8, R), rng.uniform(0, net_h - 8, R)
    props = np.stack([x1, y1, x1 + rng.uniform(4, 24, R), y1 + rng.uniform(4, 24, R)], 1).astype(np.float32)
    reg[0, 1, 2] = 30.0                                                     # r2 / 5 = 6 > log(1000 / 16)
    logits[0] = -8; logits[0, 1] = 8
    last = counts[0] - 1
    if counts[0] >= 3:
        props[last] = [net_w + 7, 5, net_w + 17, 20]; reg[last] = 0; logits[last] = -8; logits[last, 1] = 8
    if counts[0] >= 2:
        s = near_thresh + 5e-4
        logits[1] = -8; logits[1, 0] = 0
        logits[1, 1] = np.float32(math.log(s * (1 + (C - 2) * math.exp(-8)) / (1 - s)))
    return logits, reg.reshape(R, 4 * C), np.split(props, np.cumsum(counts)[:-1])

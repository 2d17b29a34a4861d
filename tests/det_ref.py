"""numpy twins of csrc/kernels_det.hip, written the slow and obvious way, and the edge masks the detection tests and
tests/golden/generate_golden_det.py share.

  instance_stats   one np.where over the frame per id (cosypose/datasets/utils.py:36-37), with the kernels' rule for values outside
                   [0, n_ids): skipped;
  box_iou          torchvision.ops.box_iou in np.float32, one operation at a time (numpy rounds every float32 operation on its own;
                   np.maximum / np.minimum propagate NaN as torch.max / torch.min / clamp do).
"""
import numpy as np

FRAMES = ((1, 1), (1, 7), (7, 1), (3, 5), (37, 53), (67, 131))


def instance_stats(masks, n_ids):
    """(B,H,W) integer masks -> (B, n_ids, 5) int32: count, x1, y1, x2, y2 (inclusive); an absent id: 0, -1, -1, -1, -1"""
    masks = np.asarray(masks)
    out = np.full((masks.shape[0], n_ids, 5), -1, dtype=np.int32)
    out[:, :, 0] = 0
    for b, mask in enumerate(masks):
        for i in np.unique(mask):
            if 0 <= i < n_ids:
                ys, xs = np.where(mask == i)
                out[b, i] = (len(ys), np.min(xs), np.min(ys), np.max(xs), np.max(ys))
    return out


def detections(masks, n_ids):
    """make_detections_from_segmentation on top of instance_stats: [{id: (x1, y1, x2, y2)}] per mask"""
    return [{int(i): tuple(int(v) for v in s[i, 1:]) for i in np.flatnonzero(s[:, 0] > 0)} for s in instance_stats(masks, n_ids)]


def box_iou(a, b):
    """(N,4), (M,4) float32 xyxy -> (N,M) float32"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all='ignore'):
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        lt = np.maximum(a[:, None, :2], b[None, :, :2])
        rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
        wh = np.maximum(rb - lt, np.float32(0))
        inter = wh[:, :, 0] * wh[:, :, 1]
        union = (area_a[:, None] + area_b[None, :]) - inter
        iou = inter / union
    assert iou.dtype == np.float32
    return iou


def box_iou_pairs(a, b):
    """(N,4), (N,4) -> (N): the same operations on the pairs alone"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all='ignore'):
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        wh = np.maximum(np.minimum(a[:, 2:], b[:, 2:]) - np.maximum(a[:, :2], b[:, :2]), np.float32(0))
        inter = wh[:, 0] * wh[:, 1]
        iou = inter / ((area_a + area_b) - inter)
    assert iou.dtype == np.float32
    return iou


def edge_masks(H, W):
    """(3,H,W) uint8, three different images: every id there is room for (all 256 from 256 pixels on) in noise; a single id; id 0 with
    id 9 at the four corner pixels only and a block of id 255 in the middle"""
    rs = np.random.RandomState(1000 * H + W)
    noise = rs.randint(0, 256, H * W)
    n = min(256, H * W)
    noise[rs.permutation(H * W)[:n]] = rs.permutation(256)[:n]
    single = np.full((H, W), 7)
    corners = np.zeros((H, W), dtype=np.int64)
    corners[H // 3:H - H // 3, W // 3:W - W // 3] = 255
    corners[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 9
    return np.stack([noise.reshape(H, W), single, corners]).astype(np.uint8)


def edge_masks_i32(H, W):
    """(3,H,W) int32 with -1, and with ids up to 1274: at or above every n_ids the tests use"""
    return edge_masks(H, W).astype(np.int32) * 5 - 1


def edge_boxes():
    """one set of boxes that holds every special case, as (a, b) pairs (n,4) float32"""
    nan, inf = np.nan, np.inf
    pairs = [
        ((10, 20, 50, 80), (10, 20, 50, 80)),                     # identical
        ((0, 0, 10, 10), (20, 20, 30, 30)),                       # disjoint
        ((0, 0, 10, 10), (10, 0, 20, 10)),                        # touching along an edge
        ((0, 0, 100, 100), (25, 30, 60, 70)),                     # contained
        ((0, 0, 10, 10), (5, 5, 5, 9)),                           # one of zero area
        ((5, 5, 5, 5), (5, 5, 5, 5)),                             # two of zero area at one point: 0 / 0
        ((50, 50, 10, 10), (0, 0, 60, 60)),                       # inverted
        ((30, 40, 10, 60), (20, 30, 40, 50)),                     # inverted along x only
        ((-50.5, -20.25, -10, -5), (-30, -15.5, 5, 0)),           # negative coordinates
        ((10000.3, 9999.7, 10050.1, 10060.9), (10010.2, 10005.5, 10070.7, 10055.3)),    # around 1e4
        ((nan, 0, 10, 10), (0, 0, 10, 10)),
        ((0, 0, 10, 10), (0, 0, nan, 10)),
        ((0, 0, inf, 10), (0, 0, 10, 10)),
        ((-inf, 0, 10, 10), (-inf, 0, 10, 10)),
        ((0, 0, inf, inf), (0, 0, inf, inf)),
        ((0.1, 0.2, 0.7, 0.9), (0.3, 0.1, 1.3, 0.6)),             # fractions that round
    ]
    a = np.array([p[0] for p in pairs], dtype=np.float32)
    b = np.array([p[1] for p in pairs], dtype=np.float32)
    return a, b


def boxes(seed, n):
    """n boxes: the special cases first (as far as n reaches), then seeded ones of all kinds"""
    rs = np.random.RandomState(seed)
    a0, b0 = edge_boxes()
    xy = rs.uniform(-50, 600, (n, 2))
    wh = rs.uniform(-20, 200, (n, 2)) * (rs.uniform(size=(n, 2)) > 0.1)      # a tenth of the sides are zero, some are negative
    a = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    shift = rs.uniform(-60, 60, (n, 2))
    wh2 = wh * rs.uniform(0.5, 1.5, (n, 2))
    b = np.concatenate([xy + shift, xy + shift + wh2], axis=1).astype(np.float32)
    k = min(n, len(a0))
    a[:k], b[:k] = a0[:k], b0[:k]
    return a, b

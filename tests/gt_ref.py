"""Numpy twin of the BOP ground-truth annotations (cosypose_amd/gt_annotations.py, csrc/kernels_gt.hip) and the hand cases the tests
share.  numpy only: nothing here imports the package or torch.  The contract is DESIGN.md section 19: the published definition of the
BOP toolkit's calc_gt_masks.py / calc_gt_info.py (visibility mode bop19) restated -- not a recording of the toolkit.

gt_info_ref takes DEPTH IMAGES, not meshes: D_gt_large (3H,3W) is the object alone on the canvas whose centre third is the frame,
D_test (H,W) the measured depth, K (3,3) the frame's unshifted intrinsics.  Distances are bop_ref.dist32 (the device's float32
arithmetic, one rounding per operation) on the crop [H:2H, W:2W]: its pixel coordinates are the integer indices of the crop, which is
x = x_canvas - W, y = y_canvas - H.  Everything must be EQUAL to the device's output.

The float64 twin (gt_info_ref(..., exact=True)) decides every pixel in float64 on the same float32 inputs and marks a pixel UNDECIDED
when dist_gt - t lies within EPS = 13 u max(dist_gt, t) of delta (bop_ref's docstring derives the 13 u: 6 u per distance and one more
rounding of the difference); dist_gt > 0, t > 0 and t == 0 are exact in both (a distance is 0 only for depth 0, NaN only for NaN).
Outside the undecided pixels the float32 and the float64 masks agree.
"""
import numpy as np

from bop_ref import dist32, dist64, U, EPS_ROUNDINGS, F32, HAND_K, HAND_HW

DELTA = 0.015


def xywh(mask, x_off=0, y_off=0):
    """[x_min, y_min, x_max - x_min, y_max - y_min] of a boolean image, the toolkit's convention (no + 1); -1 four times when empty"""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()) - x_off, int(ys.min()) - y_off, int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def gt_info_ref(D_gt_large, D_test, K, delta=DELTA, exact=False):
    """One instance -> dict(px_count_all, px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib, mask (H,W) bool,
    mask_visib (H,W) bool, undecided (H,W) bool: all False unless exact)."""
    D_gt_large, D_test = np.asarray(D_gt_large, dtype=F32), np.asarray(D_test, dtype=F32)
    H, W = D_test.shape
    assert D_gt_large.shape == (3 * H, 3 * W)
    D_gt = D_gt_large[H:2 * H, W:2 * W]
    if exact:
        dg, t, d = dist64(D_gt, K), dist64(D_test, K), float(F32(delta))
    else:
        dg, t, d = dist32(D_gt, K), dist32(D_test, K), F32(delta)
    with np.errstate(invalid='ignore'):                 # a NaN sensor value: every comparison is false
        mask = dg > 0
        valid = mask & (t > 0)
        vis = mask & (((dg - t) <= d) | (t == 0))
        undecided = np.zeros(mask.shape, dtype=bool)
        if exact:
            undecided = mask & (t > 0) & (np.abs((dg - t) - d) <= EPS_ROUNDINGS * U * np.maximum(dg, t))
    drawn = D_gt_large > 0
    n_all, n_vis = int(drawn.sum()), int(vis.sum())
    seen = n_vis > 0                                    # the toolkit's rule: no visible pixel, no boxes -- also for bbox_obj
    return dict(px_count_all=n_all, px_count_valid=int(valid.sum()), px_count_visib=n_vis, visib_fract=n_vis / n_all if n_all else 0.0,
                bbox_obj=xywh(drawn, W, H) if seen else [-1] * 4, bbox_visib=xywh(vis) if seen else [-1] * 4, mask=mask, mask_visib=vis,
                undecided=undecided)


def id_in_segm_ref(view_ids):
    """1 + the rank of every row among the rows of its view, in row order"""
    out, seen = [], {}
    for v in view_ids:
        seen[int(v)] = seen.get(int(v), 0) + 1
        out.append(seen[int(v)])
    return np.asarray(out, dtype=np.int64)


def composite_ref(masks_visib, view_ids, n_views):
    """the sequential paint of cosypose/datasets/bop.py:151-153 per view: mask[mask_n] = id_in_segm[n], rows in order -> (n_views,H,W) uint8"""
    ids = id_in_segm_ref(view_ids)
    assert len(ids) == 0 or ids.max() <= 255
    H, W = np.asarray(masks_visib).shape[1:]
    out = np.zeros((n_views, H, W), dtype=np.uint8)
    for n, v in enumerate(view_ids):
        out[int(v)][masks_visib[n]] = ids[n]
    return out


# ---- hand cases: fronto-parallel squares at z = 1 on a 48 x 64 frame (canvas 144 x 192), bop_ref.HAND_K, delta = 0.015 ------------------------
def canvas_square(z, x0, x1, y0=16, y1=32, hw=HAND_HW):
    """depth z on frame pixels [x0, x1) x [y0, y1) (frame coordinates: they may be negative or reach past the frame), as a canvas image"""
    H, W = hw
    d = np.zeros((3 * H, 3 * W), dtype=F32)
    d[H + y0:H + y1, W + x0:W + x1] = z
    return d


def crop(D_large, hw=HAND_HW):
    H, W = hw
    return D_large[H:2 * H, W:2 * W].copy()


def hand_cases():
    """-> list of (name, D_gt_large, D_test, want): want holds the exact values of the keys it names"""
    H, W = HAND_HW
    sq = canvas_square(1.0, 16, 32)
    same = crop(sq)
    half_missing = same.copy(); half_missing[:, 24:] = 0.0
    occluded = same.copy(); occluded[16:32, 24:32] = 0.9
    left = canvas_square(1.0, -8, 8)
    outside = canvas_square(1.0, -40, -24)
    nan_px = same.copy(); nan_px[20, 20] = np.nan
    full = dict(px_count_all=256, px_count_valid=256, px_count_visib=256, visib_fract=1.0, bbox_obj=[16, 16, 15, 15], bbox_visib=[16, 16, 15, 15])
    return [
        ('fully inside, sensor equal', sq, same, full),
        ('sensor 1 cm nearer', sq, np.where(same > 0, F32(0.99), 0).astype(F32), full),
        ('sensor 2 cm nearer', sq, np.where(same > 0, F32(0.98), 0).astype(F32),
         dict(px_count_all=256, px_count_valid=256, px_count_visib=0, visib_fract=0.0, bbox_obj=[-1] * 4, bbox_visib=[-1] * 4)),
        ('sensor missing on half', sq, half_missing, dict(full, px_count_valid=128)),
        ('occluder 10 cm in front of half', sq, occluded,
         dict(px_count_all=256, px_count_valid=256, px_count_visib=128, visib_fract=0.5, bbox_obj=[16, 16, 15, 15], bbox_visib=[16, 16, 7, 15])),
        ('half left of the frame', left, crop(left),
         dict(px_count_all=256, px_count_valid=128, px_count_visib=128, visib_fract=0.5, bbox_obj=[-8, 16, 15, 15], bbox_visib=[0, 16, 7, 15])),
        ('outside the frame, on the canvas', outside, np.full((H, W), 1.0, F32),
         dict(px_count_all=256, px_count_valid=0, px_count_visib=0, visib_fract=0.0, bbox_obj=[-1] * 4, bbox_visib=[-1] * 4)),
        ('one NaN sensor pixel', sq, nan_px, dict(full, px_count_valid=255, px_count_visib=255, visib_fract=255 / 256)),
    ]


def overlap_case():
    """two squares 1 cm apart that overlap on frame columns 24..31, the sensor sees the nearer one: both are visible there (1 cm < delta)
    -> (D_gt_large (2,3H,3W), D_test (H,W))"""
    a, b = canvas_square(1.0, 16, 32), canvas_square(1.01, 24, 40)
    test = np.where(crop(a) > 0, crop(a), crop(b)).astype(F32)
    return np.stack([a, b]), test

"""The twin of the backward of the multi-scale RoIAlign into the feature maps, written with detpre_ref's axis_taps and
map_levels: the forward of section 22 is the contract, this is its adjoint.  It imports nothing from cosypose_amd.

(a) roi_align_backward: derived by hand.  Per cell the terms are added in the order the contract fixes: rows ascending; inside a row the y taps
    ty = ph g + iy ascending, of one tap the low cell's weight first; inside a y entry the x taps tx = pw g + ix ascending, low first.  A term
    is fl(fl(wy wx) grad_out[r, c, ph, pw]), the sum is divided by g^2 once at the end.  float32 mode: exactly these roundings (np.add.at adds
    unbuffered, element by element in index order).  float64 mode: weights (from the float32 sample position, as roi_align64), products and
    sums in float64; it also returns sum |term| / g^2 and the number of terms per cell.
(b) adjoint_by_autograd: the forward restated as differentiable float64 torch operations (index gathers with axis_taps' indices and weights);
    torch's autograd takes its backward.  Nothing of (a) is used."""
import math

import numpy as np
import torch

import detpre_ref as pre

F = np.float32


def row_levels(boxes, im_ids, scales, B):
    """-> level per row, -1 for a row that adds nothing (image outside [0, B))"""
    k_min, k_max = int(round(-math.log2(scales[0]))), int(round(-math.log2(scales[-1])))
    levels = pre.map_levels(np.asarray(boxes, F).reshape(-1, 4), k_min, k_max)
    im_ids = np.asarray(im_ids).reshape(-1)
    return np.where((im_ids >= 0) & (im_ids < B) & (levels >= 0) & (levels < len(scales)), levels, -1)


def axis_entries(lo, hi, scale, P, g, size, dtype):
    """the entries of one axis in the contract's order -> cell, bin p, weight: per valid tap the low cell with h = 1 - l, then the high cell
    with l (a border tap with lo == hi puts both on the same cell)"""
    valid, il, ih, wl, wh = pre.axis_taps(lo, hi, scale, P, g, size)
    cell, bins, w = [], [], []
    for p in range(P):
        for i in range(g):
            if not valid[p, i]:
                continue
            l = wl[p, i] if dtype is F else np.float64(wl[p, i])
            h = wh[p, i] if dtype is F else 1 - l
            cell += [il[p, i], ih[p, i]]; bins += [p, p]; w += [h, l]
    return np.array(cell, np.int64), np.array(bins, np.int64), np.array(w, dtype)


def roi_align_backward(grad_out, boxes, im_ids, shapes, scales, P, g, B, dtype=F):
    """grad_out (R,C,P,P), boxes (R,4), im_ids (R; outside [0,B): the row adds nothing), shapes [(H_l,W_l)] -> list of (B,C,H_l,W_l) in `dtype`;
    with float64 also the lists of sum |term| / g^2 (B,C,H_l,W_l) and of the number of terms (B,H_l,W_l)"""
    grad_out = np.asarray(grad_out, F)
    R, C = grad_out.shape[:2]
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    levels = row_levels(boxes, im_ids, scales, B)
    acc = [np.zeros((B, C, H, W), dtype) for H, W in shapes]
    mag = [np.zeros((B, C, H, W), np.float64) for H, W in shapes]
    cnt = [np.zeros((B, H, W), np.int64) for H, W in shapes]
    G = grad_out if dtype is F else grad_out.astype(dtype)
    for r in range(R):
        l = int(levels[r])
        if l < 0:
            continue
        b, (H, W) = int(im_ids[r]), shapes[l]
        ys, yb, yw = axis_entries(boxes[r, 1], boxes[r, 3], scales[l], P, g, H, dtype)
        xs, xb, xw = axis_entries(boxes[r, 0], boxes[r, 2], scales[l], P, g, W, dtype)
        if len(ys) == 0 or len(xs) == 0:
            continue
        for y, ph, wy in zip(ys, yb, yw):
            w = wy * xw                                                          # fl(wy wx), (nx)
            terms = w[None, :] * G[r, :, ph, :][:, xb]                            # fl(w g), (C, nx)
            np.add.at(acc[l][b, :, y, :], (slice(None), xs), terms)              # in index order: x entries ascending, per channel
            if dtype is not F:
                np.add.at(mag[l][b, :, y, :], (slice(None), xs), np.abs(terms))
                np.add.at(cnt[l][b, y, :], xs, 1)
    count = dtype(g * g)
    if dtype is F:
        return [a / count for a in acc]
    return [a / count for a in acc], [m / count for m in mag], cnt


def forward64(features, boxes, im_ids, scales, P, g):
    """the forward of section 22 as differentiable float64 torch operations.  features: list of (B,C,H_l,W_l) float64 torch tensors -> (R,C,P,P)"""
    B, C = features[0].shape[:2]
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    levels = row_levels(boxes, im_ids, scales, B)
    out = []
    for r in range(len(boxes)):
        l = int(levels[r])
        if l < 0:
            out.append(torch.zeros((C, P, P), dtype=torch.float64))
            continue
        f = features[l][int(im_ids[r])]
        H, W = f.shape[1:]
        vy, yl, yh, ly, _ = pre.axis_taps(boxes[r, 1], boxes[r, 3], scales[l], P, g, H)
        vx, xl, xh, lx, _ = pre.axis_taps(boxes[r, 0], boxes[r, 2], scales[l], P, g, W)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
        Y0, Y1, X0, X1 = t(yl)[:, None], t(yh)[:, None], t(xl)[None, :], t(xh)[None, :]
        LY, LX = t(ly.astype(np.float64))[:, None], t(lx.astype(np.float64))[None, :]
        HY, HX = 1 - LY, 1 - LX
        ok = (t(vy)[:, None] & t(vx)[None, :]).double()
        v = (HY * HX * f[:, Y0, X0] + HY * LX * f[:, Y0, X1] + LY * HX * f[:, Y1, X0] + LY * LX * f[:, Y1, X1]) * ok        # (C, P g, P g)
        out.append(v.reshape(C, P, g, P, g).sum((2, 4)) / (g * g))
    return torch.stack(out) if out else torch.zeros((0, C, P, P), dtype=torch.float64)


def adjoint_by_autograd(grad_out, boxes, im_ids, shapes, scales, P, g, B):
    """-> list of (B,C,H_l,W_l) float64: d <forward64(F), grad_out> / d F by torch.autograd"""
    C = np.asarray(grad_out).shape[1]
    feats = [torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True) for H, W in shapes]
    out = forward64(feats, boxes, im_ids, scales, P, g)
    if out.numel() == 0 or not out.requires_grad:
        return [np.zeros((B, C, H, W)) for H, W in shapes]
    grads = torch.autograd.grad((out * torch.from_numpy(np.asarray(grad_out, np.float64))).sum(), feats, allow_unused=True)
    return [np.zeros((B, C, H, W)) if gr is None else gr.numpy() for gr, (H, W) in zip(grads, shapes)]


def padded_im_ids(B, rows, counts):
    """image of every padded row: b for the first counts[b] rows of image b, -1 for the padding"""
    ids = np.full(B * rows, -1, np.int64)
    for b in range(B):
        ids[b * rows:b * rows + min(int(counts[b]), rows)] = b
    return ids


# ---- the cases both test files run -------------------------------------------------------------------------------------------------
# section 22's small levels, in front of them one level wider than two 16-cell tiles in each axis, behind them a 1 x 1 level; two images
SHAPES = [(33, 35), (5, 7), (3, 4), (1, 2), (1, 1)]
SCALES = [2.0 ** -k for k in range(2, 7)]                                         # k_min = 2: a box below 112 px maps to level 0
B = 2
TILE = 16


def seam_boxes():
    """level-0 boxes (scale 1/4) that straddle every tile seam (cells 16 and 32) by one cell, in x, in y and in both"""
    out = []
    for sy in (None, 16, 32):
        for sx in (None, 16, 32):
            if sx is None and sy is None:
                continue
            x1, x2 = (4.0 * (sx - 1) + 1.3, 4.0 * (sx + 1) - 0.9) if sx else (21.7, 39.2)
            y1, y2 = (4.0 * (sy - 1) + 0.6, 4.0 * (sy + 1) - 1.1) if sy else (13.1, 30.4)
            out.append([x1, y1, x2, y2])
    return out


SPECIAL = seam_boxes() + [
    [10.3, 8.2, 100.7, 90.9],                                                     # level 0, over both seams of both axes
    # larger than the frame of levels 1 .. 4: both borders clamp; the last two are centred on cell 0, so that some sample lands in [-1, 1]
    [-50, -40, 100, 90], [-100, -100, 200, 250], [-334, -334, 366, 366], [-1000, -1000, 1064, 1064],
    [-9.5, 10, 18, 31], [100, -7.2, 145, 17.5], [120, 100, 150.4, 140],           # across a border of level 0
    [300, 300, 350, 350], [-70, -60, -30, -25],                                   # wholly outside: nothing
    [33.2, 14.1, 33.9, 14.6],                                                     # smaller than one cell: the clamp to 1
    [20, 20, 20, 50], [20, 20, 50, 20],                                           # zero area
    [50, 20, 20, 60], [60, 50, 20, 10],                                           # inverted in x; in both
    [0, 0, np.inf, 10], [-np.inf, 0, np.inf, 10], [5, -np.inf, 9, 7], [np.nan, 0, 10, 10], [0, 0, 10, np.nan], [np.nan] * 4]


def all_boxes(n_random=40, seed=7):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(-10, 130, n_random), rng.uniform(-10, 120, n_random)
    rand = np.stack([x1, y1, x1 + rng.uniform(2, 300, n_random), y1 + rng.uniform(2, 300, n_random)], 1)
    return np.concatenate([np.array(SPECIAL, np.float64), rand]).astype(F)


def away_from_level_boundaries(boxes, margin=1e-3):
    v = pre.level_value64(boxes)
    v = v[np.isfinite(v)]
    return bool((np.abs(v - np.round(v)) >= margin).all())


def grad_values(kind, shape, seed=0):
    if kind == 'random':
        return np.random.RandomState(100 + seed).uniform(-2, 2, shape).astype(F)
    return np.full(shape, {'zero': 0.0, 'plus': 1e4, 'minus': -1e4}[kind], F)


def make_cases():
    """-> list of dicts: name, C, P, g, boxes (R,4), im_ids (R; -1 / B: nothing) or rows + counts (padded rows), grad ('random', ...)"""
    boxes = all_boxes()
    inter = (np.arange(len(boxes)) % B).astype(np.int64)
    cases = [dict(name=f'grid C={C} P={P} g={g}', C=C, P=P, g=g, boxes=boxes, im_ids=inter, grad='random')
             for P in (1, 2, 7, 14) for g in (1, 2, 4) for C in (1, 3, 33)]
    one = np.array([[41, 41, 41.5, 41.5]], F)
    cases += [dict(name=f'{n} identical rows', C=3, P=2, g=2, boxes=np.repeat(one, n, 0), im_ids=np.zeros(n, np.int64), grad='random')
              for n in (1, 64, 65, 300)]
    cases += [dict(name=f'padded counts={c}', C=3, P=7, g=2, boxes=boxes[:16], rows=8, counts=c, grad='random') for c in ([0, 1], [1, 8], [8, 0])]
    ids = inter.copy()
    ids[[0, 5, 11]], ids[[2, 7, 12]] = -1, B
    cases.append(dict(name='image ids -1 and B', C=3, P=7, g=2, boxes=boxes, im_ids=ids, grad='random'))
    cases.append(dict(name='only level 0', C=3, P=7, g=2, boxes=boxes[:9], im_ids=inter[:9], grad='random'))
    cases += [dict(name=f'grad_out {k}', C=3, P=7, g=2, boxes=boxes, im_ids=inter, grad=k) for k in ('zero', 'plus', 'minus')]
    for i, c in enumerate(cases):
        if 'rows' in c:
            c['im_ids'] = padded_im_ids(B, c['rows'], c['counts'])
        c['grad_out'] = grad_values(c['grad'], (len(c['boxes']), c['C'], c['P'], c['P']), i)
    return cases

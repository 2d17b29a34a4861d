"""The twin of the detector's training side: torchvision 0.4.2's Matcher, BalancedPositiveNegativeSampler,
BoxCoder.encode_single, RegionProposalNetwork.compute_loss, RoIHeads.select_training_samples, fastrcnn_loss, project_masks_on_boxes and
maskrcnn_loss with Mask R-CNN's defaults, restated from the contract's text in NumPy.  It imports nothing from cosypose_amd and reads nothing
outside tests/; anchors, the RoIAlign tap rule, proposals and the multi-scale RoIAlign come from detpre_ref.py (the twin of section 22).
torchvision itself is not installed where this was written: the twin has never been run against it.

Discrete results (matches, labels, sampled sets) and the mask targets are computed in float32 with one rounding per operation, in the contract's
operation order: the kernels must reproduce them exactly.  Encodes, losses and gradients are evaluated in float64 on the same float32 inputs,
with the error bounds of section 23 beside them (`u` = 2^-24, the unit roundoff of float32)."""
import numpy as np

import detpre_ref as pre

F = np.float32
U = 2.0 ** -24
RPN_WEIGHTS, ROI_WEIGHTS = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
MAX_GRID = 4096
WEIGHTS = dict(loss_objectness=1.0, loss_rpn_box_reg=1.0, loss_classifier=1.0, loss_box_reg=1.0, loss_mask=1.0)     # h_maskrcnn's alphas


# ---- matcher -------------------------------------------------------------------------------------------------------------------------
def box_iou(gt, cand):
    """box_iou(gt (G,4), cand (N,4)) -> (G,N) float32, every operation rounded on its own; NaN, negative and -0 count as +0 (ours)"""
    a, b = np.asarray(gt, F).reshape(-1, 4), np.asarray(cand, F).reshape(-1, 4)
    with np.errstate(all='ignore'):
        area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
        h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
        w, h = np.where(w < 0, F(0), w), np.where(h < 0, F(0), h)
        inter = w * h
        v = inter / ((area_a[:, None] + area_b[None, :]) - inter)
        return np.where(v > 0, v, F(0)).astype(F)


def match(gt, cand, high, low, allow_low_quality, n_real=None):
    """Matcher -> matched (N) int64 (-1 below low, -2 between, -3 on a padding row j >= n_real), value (N) float32.  Equal IoUs: lowest g."""
    iou = box_iou(gt, cand)
    N = iou.shape[1]
    real = np.arange(N) < (N if n_real is None else n_real)
    val, arg = iou.max(0), iou.argmax(0)                                      # numpy's argmax returns the first maximum
    m = np.where(val < F(low), -1, np.where(val < F(high), -2, arg))
    if allow_low_quality:
        best = np.where(real[None], iou, F(0)).max(1)
        restore = (iou == best[:, None]).any(0)
        m = np.where(restore, arg, m)                                         # the ORIGINAL argmax, not the ground truth whose best it is
    return np.where(real, m, -3).astype(np.int64), np.where(real, val, F(0)).astype(F)


def labels_of(matched, gt_labels=None):
    """RPN (gt_labels None): 1 / 0 / -1; RoI: gt_labels[matched.clamp(0)] / 0 / -1"""
    pos = np.ones(len(matched), np.int64) if gt_labels is None else np.asarray(gt_labels, np.int64)[np.clip(matched, 0, None)]
    return np.where(matched >= 0, pos, np.where(matched == -1, 0, -1))


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
def sample(labels, keys, batch_size_per_image, positive_fraction):
    """-> all sampled indices ascending, the sampled positives ascending"""
    labels, keys = np.asarray(labels), np.asarray(keys).astype(np.int64)
    pos, neg = np.flatnonzero(labels >= 1), np.flatnonzero(labels == 0)
    n_pos = min(int(batch_size_per_image * positive_fraction), len(pos))
    n_neg = min(batch_size_per_image - n_pos, len(neg))
    take_p = np.sort(pos[np.argsort(keys[pos], kind='stable')[:n_pos]])       # stable: equal keys lower index first
    take_n = np.sort(neg[np.argsort(keys[neg], kind='stable')[:n_neg]])
    return np.sort(np.concatenate([take_p, take_n])), take_p


# ---- encode --------------------------------------------------------------------------------------------------------------------------
def encode(ref, prop, weights, dtype=F):
    """BoxCoder.encode_single in `dtype`; with float64 also the error bound of the float32 evaluation (section 23)"""
    r, p = np.asarray(ref, F).reshape(-1, 4).astype(dtype), np.asarray(prop, F).reshape(-1, 4).astype(dtype)
    wx, wy, ww, wh = (dtype(v) for v in weights)
    half = dtype(0.5)
    with np.errstate(all='ignore'):
        ew, eh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        ecx, ecy = p[:, 0] + half * ew, p[:, 1] + half * eh
        gw, gh = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        gcx, gcy = r[:, 0] + half * gw, r[:, 1] + half * gh
        out = np.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * np.log(gw / ew), wh * np.log(gh / eh)], 1)
        if dtype is F:
            return out
        # centres: 2 roundings each (extent, sum) of operands bounded by the coordinates; the difference, product and quotient one each.
        # log: the ratio carries 3 roundings, d log r = dr / r; logf within 2 ulp (HIP's documented 1, doubled); the product one.
        mag = lambda c, e: np.abs(c) + np.abs(e)
        bx = U * (np.abs(wx / ew) * 2 * (mag(gcx, gw) + mag(ecx, ew)) + 4 * np.abs(out[:, 0]))
        by = U * (np.abs(wy / eh) * 2 * (mag(gcy, gh) + mag(ecy, eh)) + 4 * np.abs(out[:, 1]))
        bw = U * (ww * (4 + 5 * np.abs(np.log(gw / ew))))
        bh = U * (wh * (4 + 5 * np.abs(np.log(gh / eh))))
        return out, np.stack([bx, by, bw, bh], 1)


# ---- loss terms in float64 -----------------------------------------------------------------------------------------------------------
def bce64(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def bce_bound(x):
    """|float32 term - float64 term|: product, difference and sum one rounding each of values up to |x| + 1; expf and log1pf within 2 ulp each
    of values <= 1 and <= ln 2, log1p's conditioning <= 1: u (4 |x| + 8)"""
    return U * (4 * np.abs(np.asarray(x, np.float64)) + 8)


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


SIGMOID_GRAD_BOUND = 8 * U        # (sigmoid(x) - y) / n: expf 2 ulp, sum, quotient, difference, quotient -> 8 u / n


def smooth_l1_64(x, beta):
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    if beta == 0:
        return ax, np.sign(x)
    return np.where(ax < beta, 0.5 * x * x / beta, ax - 0.5 * beta), np.where(ax < beta, x / beta, np.sign(x))


# ---- RPN loss ------------------------------------------------------------------------------------------------------------------------
def rpn_loss(objectness, deltas, gt_boxes, padded_size, sizes, aspect_ratios, keys, batch_size_per_image=256, positive_fraction=0.5, high=0.7,
             low=0.3):
    """objectness[l] (B,A,H,W), deltas[l] (B,4A,H,W) float32 arrays, gt_boxes [(G_i,4)], keys (B,N) -> dict: losses and their bounds (float64),
    grad_objectness / grad_deltas (lists in the heads' layouts, float64), matched (B,N), sampled [(n_b)]"""
    B = objectness[0].shape[0]
    anchors = pre.anchors([o.shape[2:] for o in objectness], padded_size, sizes, aspect_ratios)
    g_obj, g_dl = [np.zeros(o.shape) for o in objectness], [np.zeros(d.shape) for d in deltas]
    per_image, n_s = [], 0
    for b in range(B):
        m, _ = match(gt_boxes[b], anchors, high, low, True)
        samp, _ = sample(labels_of(m), keys[b], batch_size_per_image, positive_fraction)
        per_image.append((m, samp))
        n_s += len(samp)
    t_obj = b_obj = t_box = b_box = 0.0
    for b, (m, samp) in enumerate(per_image):
        flat = [pre.flatten_level(np.asarray(o[b], F), np.asarray(d[b], F)) for o, d in zip(objectness, deltas)]
        logits, rel = np.concatenate([f[0] for f in flat]), np.concatenate([f[1] for f in flat])
        y = (m[samp] >= 0).astype(np.float64)
        x = logits[samp]
        t_obj += bce64(x, y).sum(); b_obj += bce_bound(x).sum()
        go = np.zeros(len(logits)); go[samp] = (sigmoid64(x) - y) / n_s
        posi = samp[m[samp] >= 0]
        t64, tb = encode(np.asarray(gt_boxes[b], F)[m[posi]], anchors[posi], RPN_WEIGHTS, np.float64)
        diff = rel[posi].astype(np.float64) - t64
        t_box += np.abs(diff).sum(); b_box += (tb + U * np.abs(diff)).sum()
        gd = np.zeros(rel.shape); gd[posi] = np.sign(diff) / n_s
        first = 0
        for l, o in enumerate(objectness):
            A, H, W = o.shape[1:]
            n = A * H * W
            g_obj[l][b] = go[first:first + n].reshape(H, W, A).transpose(2, 0, 1)
            g_dl[l][b] = gd[first:first + n].reshape(H, W, A, 4).transpose(2, 3, 0, 1).reshape(4 * A, H, W)
            first += n
    losses = dict(loss_objectness=t_obj / n_s, loss_rpn_box_reg=t_box / n_s)
    bounds = dict(loss_objectness=b_obj / n_s + U * abs(losses['loss_objectness']), loss_rpn_box_reg=b_box / n_s + U * abs(losses['loss_rpn_box_reg']))
    return dict(losses=losses, bounds=bounds, grad_objectness=g_obj, grad_deltas=g_dl, matched=np.stack([p[0] for p in per_image]),
                sampled=[p[1] for p in per_image], n_sampled=n_s)


# ---- RoI training samples --------------------------------------------------------------------------------------------------------------
def roi_samples(proposals, gt_boxes, gt_labels, keys, rows, G_max, batch_size_per_image=512, positive_fraction=0.25, high=0.5, low=0.5,
                weights=ROI_WEIGHTS):
    """one image: proposals (n,4) real rows.  Candidates as the kernels index them: the proposals, the ground truths, zero rows up to rows +
    G_max.  -> dict of the sampled rows (ascending candidate index) and the positives among them"""
    prop, gt = np.asarray(proposals, F).reshape(-1, 4), np.asarray(gt_boxes, F).reshape(-1, 4)
    N = rows + G_max
    cand = np.zeros((N, 4), F)
    n = len(prop) + len(gt)
    cand[:len(prop)], cand[len(prop):n] = prop, gt
    m, _ = match(gt, cand, high, low, False, n)
    lab = labels_of(m, gt_labels)
    samp, pos = sample(lab, keys, batch_size_per_image, positive_fraction)
    cl = np.clip(m, 0, None)
    t64, tb = encode(gt[cl[samp]], cand[samp], weights, np.float64)
    return dict(idx=samp, boxes=cand[samp], labels=lab[samp], matched=cl[samp], targets64=t64, target_bounds=tb, pos_idx=pos, pos_boxes=cand[pos],
                pos_labels=lab[pos], pos_matched=cl[pos], all_matched=m, all_labels=lab)


# ---- Fast R-CNN loss ---------------------------------------------------------------------------------------------------------------------
def fastrcnn_loss(class_logits, box_regression, labels, targets):
    """float64 on the float32 inputs; rows with label < 0 are padding -> losses, bounds, grad_logits (R,C), grad_box (R,4C), grad bounds"""
    z, d = np.asarray(class_logits, F).astype(np.float64), np.asarray(box_regression, F).astype(np.float64)
    labels, t = np.asarray(labels, np.int64), np.asarray(targets, F).astype(np.float64)
    R, C = z.shape
    real = labels >= 0
    n = int(real.sum())
    gz, gd = np.zeros((R, C)), np.zeros((R, 4 * C))
    ce = b_ce = l1 = b_l1 = 0.0
    g_bound = np.zeros((R, 1))
    for r in np.flatnonzero(real):
        mx = z[r].max()
        e = np.exp(z[r] - mx)
        s = e.sum()
        ce += np.log(s) - (z[r, labels[r]] - mx)
        # z - max: one rounding of up to D = the largest distance that still contributes (exp > 0: at most 104); expf 2 ulp; C / 64 + 6 sums;
        # logf 2 ulp and the conditioning of log (1): u (2 D + 12 + 4 |log s|); the label's difference and the final one: u |z_label - max| twice
        D = min(104.0, float((mx - z[r]).max()))
        b_ce += U * (2 * D + 12 + C / 64 + 4 * abs(np.log(s)) + 2 * abs(z[r, labels[r]] - mx))
        p = e / s
        p[labels[r]] -= 1
        gz[r] = p / n
        g_bound[r] = U * (2 * D + 16 + C / 64) / n
        if labels[r] > 0:
            diff = d[r, 4 * labels[r]:4 * labels[r] + 4] - t[r]
            v, g = smooth_l1_64(diff, 1.0)
            l1 += v.sum(); b_l1 += (4 * U * (np.abs(diff) + diff * diff)).sum()
            gd[r, 4 * labels[r]:4 * labels[r] + 4] = g / n
    n_div = max(n, 1)
    losses = dict(loss_classifier=ce / n_div, loss_box_reg=l1 / n_div)
    bounds = dict(loss_classifier=b_ce / n_div + U * abs(losses['loss_classifier']), loss_box_reg=b_l1 / n_div + U * abs(losses['loss_box_reg']))
    return dict(losses=losses, bounds=bounds, grad_logits=gz, grad_box=gd, grad_logits_bound=g_bound, grad_box_bound=4 * U / n_div, n=n)


# ---- mask targets and loss ---------------------------------------------------------------------------------------------------------------
def adaptive_grid(lo, hi, M):
    """g = ceil(max(extent, 1) / M) in float32, capped at MAX_GRID (ours); NaN -> 1"""
    with np.errstate(all='ignore'):
        ext = F(hi) - F(lo)
        size = ext if ext > F(1) else F(1)
        g = np.ceil(size / F(M))
    return int(min(g, MAX_GRID)) if g >= 1 else 1


def mask_target(mask, box, M):
    """one RoI: mask (H,W) uint8, box (4) -> (M,M) float32, bit for bit what the contract's operation order gives: iy outer, ix inner, each sample
    w1 p1 + w2 p2 + w3 p3 + w4 p4 left to right, the sum divided by g_h g_w"""
    mask = np.asarray(mask).astype(F)
    H, W = mask.shape
    box = np.asarray(box, F)
    gh, gw = adaptive_grid(box[1], box[3], M), adaptive_grid(box[0], box[2], M)
    vy, yl, yh, ly, hy = pre.axis_taps(box[1], box[3], 1.0, M, gh, H)
    vx, xl, xh, lx, hx = pre.axis_taps(box[0], box[2], 1.0, M, gw, W)
    acc = np.zeros((M, M), F)
    for iy in range(gh):
        for ix in range(gw):
            ok = vy[:, iy][:, None] & vx[:, ix][None, :]
            Y0, Y1, X0, X1 = yl[:, iy][:, None], yh[:, iy][:, None], xl[:, ix][None, :], xh[:, ix][None, :]
            HY, LY, HX, LX = hy[:, iy][:, None], ly[:, iy][:, None], hx[:, ix][None, :], lx[:, ix][None, :]
            w1, w2, w3, w4 = HY * HX, HY * LX, LY * HX, LY * LX
            v = ((w1 * mask[Y0, X0] + w2 * mask[Y0, X1]) + w3 * mask[Y1, X0]) + w4 * mask[Y1, X1]
            acc = np.where(ok, acc + v, acc)
    return (acc / (F(gh) * F(gw))).astype(F)


def mask_targets(masks, boxes, matched, M):
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    out = np.zeros((len(boxes), M, M), F)
    for r, (box, g) in enumerate(zip(boxes, matched)):
        if 0 <= g < len(masks):
            out[r] = mask_target(masks[g], box, M)
    return out


def mask_loss(mask_logits, labels, targets, real):
    """float64 BCE of mask_logits[r, label_r] (R,C,M,M float32) against targets (R,M,M, the float32 twin's) over the real rows -> loss, bound,
    grad (R,C,M,M), n_pos"""
    x_all = np.asarray(mask_logits, F).astype(np.float64)
    R, C, M, _ = x_all.shape
    grad = np.zeros(x_all.shape)
    rows = np.flatnonzero(real)
    n = len(rows)
    if n == 0:
        return 0.0, 0.0, grad, 0
    tot = bound = 0.0
    for r in rows:
        x, t = x_all[r, labels[r]], np.asarray(targets[r], np.float64)
        tot += bce64(x, t).sum(); bound += bce_bound(x).sum()
        grad[r, labels[r]] = (sigmoid64(x) - t) / (n * M * M)
    loss = tot / (n * M * M)
    return loss, bound / (n * M * M) + U * abs(loss), grad, n


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def chain(features, heads, targets, net_sizes, padded_size, sizes, aspect_ratios, keys, n_roi_levels, rpn_options, bs=512, frac=0.25):
    """the twin of detector_losses over numpy features; heads = (rpn_head, box_head, mask_head), callables over numpy arrays -> dict with the
    five losses (float64), their bounds, and the gradients at the heads' raw outputs"""
    rpn_head, box_head, mask_head = heads
    objectness, deltas = rpn_head(features)
    B = objectness[0].shape[0]
    gt = [np.asarray(t['boxes'], F) for t in targets]
    rpn = rpn_loss(objectness, deltas, gt, padded_size, sizes, aspect_ratios, keys['rpn'])
    props = pre.proposals(objectness, deltas, net_sizes, padded_size, sizes, aspect_ratios, **rpn_options)
    rows, G_max, n_pos_max = rpn_options['post_nms_top_n'], max(len(g) for g in gt), int(bs * frac)
    smp = [roi_samples(props[b]['boxes'], gt[b], targets[b]['labels'], keys['roi'][b], rows, G_max, bs, frac) for b in range(B)]
    roi_maps = features[:n_roi_levels]
    scales = pre.infer_scales([f.shape[2:] for f in roi_maps], net_sizes)
    boxes, labels, t64, real = np.zeros((B * bs, 4), F), np.full(B * bs, -1, np.int64), np.zeros((B * bs, 4)), np.zeros(B * bs, bool)
    pbox, plab, pm, preal = np.zeros((B * n_pos_max, 4), F), np.zeros(B * n_pos_max, np.int64), np.zeros(B * n_pos_max, np.int64), np.zeros(B * n_pos_max, bool)
    for b, s in enumerate(smp):
        n, k = len(s['idx']), len(s['pos_idx'])
        boxes[b * bs:b * bs + n], labels[b * bs:b * bs + n], t64[b * bs:b * bs + n], real[b * bs:b * bs + n] = s['boxes'], s['labels'], s['targets64'], True
        pbox[b * n_pos_max:b * n_pos_max + k], plab[b * n_pos_max:b * n_pos_max + k], pm[b * n_pos_max:b * n_pos_max + k] = s['pos_boxes'], s['pos_labels'], s['pos_matched']
        preal[b * n_pos_max:b * n_pos_max + k] = True
    C = roi_maps[0].shape[1]
    feats = np.zeros((B * bs, C, 7, 7), F)                                    # a padding row: zero features, as the device chain hands them on
    feats[real] = pre.multiscale_roi_align(roi_maps, boxes[real], np.repeat(np.arange(B), bs)[real], scales, 7, 2)[0]
    class_logits, box_regression = box_head(feats)
    frc = fastrcnn_loss(class_logits, box_regression, labels, t64.astype(F))
    mfeats = np.zeros((B * n_pos_max, C, 14, 14), F)
    mfeats[preal] = pre.multiscale_roi_align(roi_maps, pbox[preal], np.repeat(np.arange(B), n_pos_max)[preal], scales, 14, 2)[0]
    mask_logits = mask_head(mfeats)
    M = mask_logits.shape[-1]
    tg = np.zeros((B * n_pos_max, M, M), F)
    for r in np.flatnonzero(preal):
        tg[r] = mask_target(np.asarray(targets[r // n_pos_max]['masks'])[pm[r]], pbox[r], M)
    ml, mb, mg, _ = mask_loss(mask_logits, plab, tg, preal)
    losses = dict(rpn['losses'], **frc['losses'], loss_mask=ml)
    bounds = dict(rpn['bounds'], **frc['bounds'], loss_mask=mb)
    # in the chain the regression targets are the float32 encode's, not inputs: their own bound enters the box loss (|d smooth_l1| <= 1)
    t_bound = np.zeros((B * bs, 4))
    for b, s in enumerate(smp):
        t_bound[b * bs:b * bs + len(s['idx'])] = s['target_bounds']
    bounds['loss_box_reg'] += t_bound[labels > 0].sum() / max(frc['n'], 1)
    return dict(losses=losses, bounds=bounds, rpn=rpn, frc=frc, grad_mask=mg, samples=smp, target_bounds=t_bound, labels=labels, pos_labels=plab, pos_real=preal)

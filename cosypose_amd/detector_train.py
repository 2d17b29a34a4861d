"""Training side of the detector: from the heads' raw outputs and the targets to the `loss_dict` the reference's h_maskrcnn
(cosypose/training/maskrcnn_forward_loss.py) gets from `model(images, targets)`: loss_objectness, loss_rpn_box_reg, loss_classifier,
loss_box_reg, loss_mask.  What torchvision 0.4.2 (Matcher, BalancedPositiveNegativeSampler, BoxCoder.encode, RegionProposalNetwork.compute_loss,
RoIHeads.select_training_samples, fastrcnn_loss, project_masks_on_boxes, maskrcnn_loss) does around the convolutions; the convolutions and
linears stay ordinary torch.nn modules.  DESIGN.md section 23 states the contract; HIP: csrc/kernels_dettrain.hip.

What runs where
  * device, our kernels: the match of every anchor / proposal against the ground truths (cosy_dt_match), the balanced subsample
    (cosy_dt_sample), the RPN losses with their gradients (cosy_dt_rpn_loss), proposals + ground truths -> sampled RoIs with labels and
    regression targets (cosy_dt_roi_candidates, cosy_dt_roi_gather), the Fast R-CNN losses (cosy_dt_fastrcnn_loss), mask targets from the uint8
    masks and the mask loss (cosy_dt_mask_loss);
  * device, torch as plumbing: torch.randint for the sampler's keys when none are passed, torch.cat of the images' few ground-truth boxes,
    zero-filled gradient tensors for the RPN, grad_output x stored gradient in backward;
  * host: the level description (section 22), the ground-truth counts (known from the shapes).  No device-to-host copy anywhere.

Targets: one dict per image with boxes (G_i,4) float32 xyxy, labels (G_i) int64 >= 1, masks (G_i,H,W) uint8, on the device, in the
coordinates of the image as the network saw it.  An image without a ground truth is refused (torchvision 0.4.2's Matcher refuses it).
Rows are PADDED as in detector_rpn: image b owns rows [b n, (b+1) n), its first counts[b] are real; a padding row has a zero box and label -1.
No gradient flows into targets, proposals, keys or the feature maps (the RoIAlign of section 22 has no backward).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import detector
from . import detector_rpn
from .detector import MAX_CLASSES, MAX_IMAGES             # COSY_DT_MAX_CLASSES; the images of one call, as on every side of the detector
from .detector_rpn import DEFAULT_SIZES, DEFAULT_RATIOS, AnchorGrid

MAX_GT = _lib.DT_MAX_GT          # ground truths per image (they sit in LDS)
MAX_BATCH = _lib.DT_MAX_BATCH    # batch_size_per_image
MAX_MASK_SIDE = _lib.DT_MAX_M
RPN_WEIGHTS, ROI_WEIGHTS = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
LOSS_KEYS = ('loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg', 'loss_mask')


# ---- argument checks: all of them run before the library is loaded -----------------------------------------------------------------
def _gt_list(gt_boxes, name='gt_boxes'):
    if torch.is_tensor(gt_boxes):
        gt_boxes = [gt_boxes]
    if not isinstance(gt_boxes, (list, tuple)) or not gt_boxes:
        raise ValueError(f'{name} must be a non-empty list of (G_i,4) tensors, one per image')
    out = [detector._tensor(g, f'{name}[{i}]', (None, 4)) for i, g in enumerate(gt_boxes)]
    if len(out) > MAX_IMAGES:
        raise ValueError(f'{len(out)} images exceed the limit of {MAX_IMAGES} per call')
    for i, g in enumerate(out):
        if g.shape[0] == 0:
            raise ValueError(f'{name}[{i}] holds no ground truth: an image without one is refused (as torchvision 0.4.2\'s Matcher refuses it)')
        if g.shape[0] > MAX_GT:
            raise ValueError(f'{name}[{i}] holds {g.shape[0]} ground truths, the limit is {MAX_GT} per image')
    return out


def _targets(targets, B=None, masks=False):
    """-> boxes [(G_i,4)], labels [(G_i) int32][, masks [(G_i,H,W) uint8]]"""
    if not isinstance(targets, (list, tuple)) or not targets or not all(isinstance(t, dict) for t in targets):
        raise ValueError('targets must be a non-empty list of dicts (boxes, labels, masks), one per image')
    if B is not None and len(targets) != B:
        raise ValueError(f'targets must hold one dict per image: {B} images, got {len(targets)}')
    boxes = _gt_list([t['boxes'] for t in targets], 'targets boxes')
    labels = []
    for i, (t, bx) in enumerate(zip(targets, boxes)):
        labels.append(detector._int_tensor(t['labels'], f'targets[{i}] labels', int(bx.shape[0])))
    if not masks:
        return boxes, labels
    out = []
    for i, (t, bx) in enumerate(zip(targets, boxes)):
        m = detector._tensor(t['masks'], f'targets[{i}] masks', (int(bx.shape[0]), None, None), torch.uint8)
        if m.shape[1] < 1 or m.shape[2] < 1 or m.shape[1] * m.shape[2] >= 1 << 30:
            raise ValueError(f'targets[{i}] masks must have 1 <= H W < 2^30 pixels, got {tuple(m.shape)}')
        out.append(m)
    return boxes, labels, out


def _sampler_args(batch_size_per_image, positive_fraction):
    bs, frac = int(batch_size_per_image), float(positive_fraction)
    if not 1 <= bs <= MAX_BATCH:
        raise ValueError(f'batch_size_per_image must lie in [1, {MAX_BATCH}], got {batch_size_per_image}')
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f'positive_fraction must lie in [0, 1], got {positive_fraction}')
    return bs, int(bs * frac)


def _keys(keys, B, N):
    return None if keys is None else detector._tensor(keys, 'keys', (B, N), torch.int32)


def _draw_keys(keys, B, N, device, generator):
    """the sampler's keys: the caller's, or non-negative int32 drawn on the device"""
    if keys is not None:
        return keys
    return torch.randint(0, 2 ** 31 - 1, (B, N), dtype=torch.int32, device=device, generator=generator)


def _weights(weights):
    w = tuple(float(v) for v in weights)
    if len(w) != 4:
        raise ValueError(f'weights must hold four numbers (wx, wy, ww, wh), got {weights}')
    return w


def _gt_device(boxes, labels, dev):
    """concatenated ground truths: boxes (G_total,4), labels (G_total) int32 or None, offsets (B+1) int32 on the device, G_max, G_total"""
    G = [int(b.shape[0]) for b in boxes]
    off = _lib.ints_to_device(np.concatenate([[0], np.cumsum(G)]), dev)
    gt = torch.cat(boxes) if len(boxes) > 1 else boxes[0]
    lab = None if labels is None else (torch.cat(labels) if len(labels) > 1 else labels[0])
    return gt, lab, off, max(G), sum(G)


# ---- matcher -------------------------------------------------------------------------------------------------------------------------
def _match(grid, cand, cand_counts, N, gt, gt_lab, gt_off, G_max, G_total, B, high, low, allow_low_quality, want_labels):
    dev = gt.device
    matched = torch.empty((B, N), dtype=torch.int32, device=dev)
    iou = torch.empty((B, N), dtype=torch.float32, device=dev)
    labels = torch.empty((B, N), dtype=torch.int32, device=dev) if want_labels else None
    best = torch.empty(G_total, dtype=torch.int32, device=dev) if allow_low_quality else None
    lv = grid.levels() if grid is not None else None
    _lib.check(_lib.lib().cosy_dt_match(ctypes.byref(lv) if lv is not None else None, grid.L if grid else 0, grid.A if grid else 0, _lib.ptr(cand),
                                        _lib.ptr(cand_counts), N, B, _lib.ptr(gt), _lib.ptr(gt_off), _lib.ptr(gt_lab), G_max, G_total, float(high),
                                        float(low), int(bool(allow_low_quality)), _lib.ptr(best), _lib.ptr(matched), _lib.ptr(iou), _lib.ptr(labels),
                                        _lib.stream()))
    return matched, iou, labels


def match_boxes(gt_boxes, candidates, high_threshold, low_threshold, allow_low_quality_matches=False, counts=None, gt_labels=None):
    """Matcher(high, low, allow_low_quality_matches) over box_iou(gt, candidates), all images at once.
    gt_boxes: list of (G_i,4) float32 device tensors, one per image (a single tensor: one image).  candidates: an AnchorGrid (the anchors are
    formed from their index, the same for every image) or a (B,N,4) float32 device tensor of padded rows, of which image b's first counts[b]
    ((B) int32 device tensor; None: all) are candidates.  gt_labels: list of (G_i) int tensors -> also the labels.
    -> matched_idxs (B,N) int32: the ground truth's index, -1 below low, -2 between, -3 on a padding row; matched_iou (B,N) float32[; labels
    (B,N) int32: gt_labels[matched] / 0 / -1 (ignored)].  Equal IoUs go to the lowest ground truth; a NaN IoU counts as 0."""
    boxes = _gt_list(gt_boxes)
    B = len(boxes)
    high, low = float(high_threshold), float(low_threshold)
    if not low <= high:
        raise ValueError(f'low_threshold = {low_threshold} must not exceed high_threshold = {high_threshold}')
    labels = None
    if gt_labels is not None:
        if torch.is_tensor(gt_labels):
            gt_labels = [gt_labels]
        if len(gt_labels) != B:
            raise ValueError(f'gt_labels must hold one tensor per image: {B} images, got {len(gt_labels)}')
        labels = [detector._int_tensor(l, f'gt_labels[{i}]', int(b.shape[0])) for i, (l, b) in enumerate(zip(gt_labels, boxes))]
    grid = cand = None
    if isinstance(candidates, AnchorGrid):
        grid, N = candidates, candidates.N
        if counts is not None:
            raise ValueError('counts go with a tensor of candidate boxes, not with an AnchorGrid')
    else:
        cand = detector._tensor(candidates, 'candidates', (B, None, 4))
        N = int(cand.shape[1])
        if N < 1:
            raise ValueError('candidates must hold at least one row per image')
        if counts is not None:
            counts = detector._int_tensor(counts, 'counts', B)
    detector._on_device(gt_boxes=boxes, gt_labels=labels, candidates=cand, counts=counts)
    gt, lab, off, G_max, G_total = _gt_device(boxes, labels, boxes[0].device)
    matched, iou, out_labels = _match(grid, cand, counts, N, gt, lab, off, G_max, G_total, B, high, low, allow_low_quality_matches, labels is not None)
    return (matched, iou, out_labels) if labels is not None else (matched, iou)


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
def _sample(labels, keys, B, N, bs, n_pos_max):
    dev = labels.device
    samp_idx = torch.full((B, bs), -1, dtype=torch.int32, device=dev)
    pos_idx = torch.full((B, max(n_pos_max, 1)), -1, dtype=torch.int32, device=dev)
    samp_count = torch.empty(B, dtype=torch.int32, device=dev)
    pos_count = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().cosy_dt_sample(_lib.ptr(labels), _lib.ptr(keys), N, B, bs, n_pos_max, _lib.ptr(samp_idx), _lib.ptr(samp_count), _lib.ptr(pos_idx),
                                         _lib.ptr(pos_count), _lib.stream()))
    return samp_idx, samp_count, pos_idx[:, :n_pos_max], pos_count


def sample_balanced(labels, batch_size_per_image, positive_fraction, keys=None, generator=None):
    """BalancedPositiveNegativeSampler: labels (B,N) int32 on the device (>= 1 positive, 0 negative, < 0 ignored).  n_pos = min(int(bs frac),
    P), n_neg = min(bs - n_pos, N).  Every candidate carries a non-negative int32 key (keys (B,N); None: torch.randint on the device from
    `generator`): the n_pos positives and the n_neg negatives with the smallest keys are taken, equal keys lower index first.
    -> samp_idx (B,bs) int32: the sampled indices in ascending order, -1 past samp_count (B); pos_idx (B, int(bs frac)), pos_count (B): the
    sampled positives.  P, N and the cuts are decided on the device."""
    if not torch.is_tensor(labels) or labels.dim() != 2:
        raise ValueError(f'labels must be a (B,N) tensor, got {tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__}')
    B, N = int(labels.shape[0]), int(labels.shape[1])
    labels = detector._tensor(labels, 'labels', (B, N), torch.int32)
    if not 1 <= B <= MAX_IMAGES or N < 1:
        raise ValueError(f'labels must hold 1 to {MAX_IMAGES} images of at least one candidate, got {(B, N)}')
    bs, n_pos_max = _sampler_args(batch_size_per_image, positive_fraction)
    keys = _keys(keys, B, N)
    detector._on_device(labels=labels, keys=keys)
    keys = _draw_keys(keys, B, N, labels.device, generator)
    return _sample(labels, keys, B, N, bs, n_pos_max)


# ---- encode --------------------------------------------------------------------------------------------------------------------------
def encode_boxes(reference_boxes, proposals, weights=ROI_WEIGHTS):
    """BoxCoder.encode_single: the regression targets (n,4) that take `proposals` (n,4) to `reference_boxes` (n,4); a zero extent gives the
    IEEE result (inf / NaN)"""
    proposals = detector._tensor(proposals, 'proposals', (None, 4))
    reference_boxes = detector._tensor(reference_boxes, 'reference_boxes', (int(proposals.shape[0]), 4))
    w = _weights(weights)
    detector._on_device(reference_boxes=reference_boxes, proposals=proposals)
    out = torch.empty_like(proposals)
    _lib.check(_lib.lib().cosy_dt_encode(_lib.ptr(reference_boxes), _lib.ptr(proposals), int(proposals.shape[0]), *w, _lib.ptr(out), _lib.stream()))
    return out


# ---- RPN losses ------------------------------------------------------------------------------------------------------------------------
class _RpnLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *heads):
        grid, B, bs, samp_idx, samp_count, matched, gt, gt_off = meta
        L = grid.L
        obj, dl = [h.detach() for h in heads[:L]], [h.detach() for h in heads[L:]]
        dev = obj[0].device
        g_obj, g_dl = [torch.zeros_like(o) for o in obj], [torch.zeros_like(d) for d in dl]
        lv, gr = grid.levels(obj, dl), grid.levels(g_obj, g_dl)
        terms = torch.empty(2 * B * bs, dtype=torch.float64, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().cosy_dt_rpn_loss(ctypes.byref(lv), ctypes.byref(gr), L, grid.A, B, bs, _lib.ptr(samp_idx), _lib.ptr(samp_count),
                                               _lib.ptr(matched), _lib.ptr(gt), _lib.ptr(gt_off), _lib.ptr(terms), _lib.ptr(losses), _lib.stream()))
        ctx.grads = (g_obj, g_dl)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, d_obj, d_box):
        g_obj, g_dl = ctx.grads
        return (None,) + tuple(g * d_obj for g in g_obj) + tuple(g * d_box for g in g_dl)


def rpn_loss(objectness, bbox_deltas, targets, net_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS, keys=None, generator=None,
             batch_size_per_image=256, positive_fraction=0.5, fg_iou_thresh=0.7, bg_iou_thresh=0.3, return_samples=False):
    """RegionProposalNetwork.compute_loss of torchvision 0.4.2 over the RPN head's raw outputs, all images and levels at once: the match of
    every anchor (no visibility filter) with Matcher(0.7, 0.3, True), the balanced subsample (256, 0.5), the encode with weights 1, then
    loss_objectness = mean BCE-with-logits over the sampled anchors and loss_rpn_box_reg = sum |d - t| over the sampled positives / the sampled
    (plain L1: 0.4.2).  objectness[l] (B,A,H_l,W_l), bbox_deltas[l] (B,4A,H_l,W_l): float32, contiguous, on the device, read in place; keys
    (B, anchors per image) int32 or None.  -> (loss_objectness, loss_rpn_box_reg), differentiable with respect to the head's outputs[, and
    with return_samples (matched_idxs, samp_idx, samp_count)]."""
    objectness, bbox_deltas, B, A, _ = detector_rpn._rpn_heads(objectness, bbox_deltas)
    grid = detector_rpn._rpn_grid(objectness, A, padded_size, sizes, aspect_ratios)
    boxes, _ = _targets(targets, B)
    detector._sizes(net_sizes, 'net_sizes', B)
    bs, n_pos_max = _sampler_args(batch_size_per_image, positive_fraction)
    keys = _keys(keys, B, grid.N)
    detector._on_device(objectness=objectness, bbox_deltas=bbox_deltas, gt_boxes=boxes, keys=keys)
    dev = objectness[0].device
    gt, _, off, G_max, G_total = _gt_device(boxes, None, dev)
    matched, _, labels = _match(grid, None, None, grid.N, gt, None, off, G_max, G_total, B, fg_iou_thresh, bg_iou_thresh, True, True)
    samp_idx, samp_count, _, _ = _sample(labels, _draw_keys(keys, B, grid.N, dev, generator), B, grid.N, bs, n_pos_max)
    losses = _RpnLossFn.apply((grid, B, bs, samp_idx, samp_count, matched, gt, off), *objectness, *bbox_deltas)
    return losses + ((matched, samp_idx, samp_count),) if return_samples else losses


# ---- RoI training samples --------------------------------------------------------------------------------------------------------------
def roi_training_samples(proposals, counts, targets, keys=None, generator=None, batch_size_per_image=512, positive_fraction=0.25, fg_iou_thresh=0.5,
                         bg_iou_thresh=0.5, weights=ROI_WEIGHTS):
    """RoIHeads.select_training_samples: proposals (B rows, 4) padded rows with counts (B) int32 on the device (rpn_proposals' layout).  The
    ground-truth boxes are appended to each image's proposals (candidate index: the proposals, then the ground truths, then padding up to rows +
    max G), matched with Matcher(0.5, 0.5, False), labelled, subsampled (512, 0.25; keys (B, rows + max G) int32 or None), and the sampled rows,
    in ascending candidate index, encoded against their matched ground truth with weights (10, 10, 5, 5).
    -> dict: boxes (B bs,4), labels (B bs) int32 (-1: padding), matched_idxs (B bs) int32 (clamped at 0), regression_targets (B bs,4), counts (B);
    pos_boxes (B n,4), pos_labels, pos_matched_idxs (B n), pos_counts (B) with n = int(bs frac): the sampled positives, for the mask branch."""
    boxes, labels = _targets(targets)
    B = len(boxes)
    proposals = detector._tensor(proposals, 'proposals', (None, 4))
    counts = detector._int_tensor(counts, 'counts', B)
    if proposals.shape[0] % B:
        raise ValueError(f'proposals are padded rows, the same number for each of the {B} images: got {proposals.shape[0]} rows')
    rows = int(proposals.shape[0]) // B
    bs, n_pos_max = _sampler_args(batch_size_per_image, positive_fraction)
    w = _weights(weights)
    G_max = max(int(b.shape[0]) for b in boxes)
    N = rows + G_max
    keys = _keys(keys, B, N)
    detector._on_device(proposals=proposals, counts=counts, gt_boxes=boxes, gt_labels=labels, keys=keys)
    dev = proposals.device
    gt, lab, off, G_max, G_total = _gt_device(boxes, labels, dev)
    l_ = _lib.lib()
    cand = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    cand_counts = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(l_.cosy_dt_roi_candidates(_lib.ptr(proposals), _lib.ptr(counts), rows, _lib.ptr(gt), _lib.ptr(off), B, G_max, _lib.ptr(cand),
                                         _lib.ptr(cand_counts), _lib.stream()))
    matched, _, cand_labels = _match(None, cand, cand_counts, N, gt, lab, off, G_max, G_total, B, fg_iou_thresh, bg_iou_thresh, False, True)
    samp_idx, samp_count, pos_idx, pos_count = _sample(cand_labels, _draw_keys(keys, B, N, dev, generator), B, N, bs, n_pos_max)
    pos_idx = pos_idx.contiguous()
    out = dict(boxes=torch.empty((B * bs, 4), dtype=torch.float32, device=dev), labels=torch.empty(B * bs, dtype=torch.int32, device=dev),
               matched_idxs=torch.empty(B * bs, dtype=torch.int32, device=dev), regression_targets=torch.empty((B * bs, 4), dtype=torch.float32, device=dev),
               counts=samp_count, pos_boxes=torch.empty((B * n_pos_max, 4), dtype=torch.float32, device=dev),
               pos_labels=torch.empty(B * n_pos_max, dtype=torch.int32, device=dev), pos_matched_idxs=torch.empty(B * n_pos_max, dtype=torch.int32, device=dev),
               pos_counts=pos_count)
    _lib.check(l_.cosy_dt_roi_gather(_lib.ptr(cand), N, _lib.ptr(matched), _lib.ptr(cand_labels), _lib.ptr(samp_idx), _lib.ptr(samp_count), _lib.ptr(pos_idx),
                                     _lib.ptr(pos_count), _lib.ptr(gt), _lib.ptr(off), B, bs, n_pos_max, *w, _lib.ptr(out['boxes']), _lib.ptr(out['labels']),
                                     _lib.ptr(out['matched_idxs']), _lib.ptr(out['regression_targets']), _lib.ptr(out['pos_boxes']),
                                     _lib.ptr(out['pos_labels']), _lib.ptr(out['pos_matched_idxs']), _lib.stream()))
    return out


# ---- Fast R-CNN losses -------------------------------------------------------------------------------------------------------------------
class _FastRcnnLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, class_logits, box_regression, labels, regression_targets):
        z, d = class_logits.detach().contiguous(), box_regression.detach().contiguous()
        R, C = int(z.shape[0]), int(z.shape[1])
        dev = z.device
        g_z, g_d = torch.empty_like(z), torch.empty_like(d)
        n_real = torch.empty(1, dtype=torch.int32, device=dev)
        terms = torch.empty(2 * R, dtype=torch.float64, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().cosy_dt_fastrcnn_loss(_lib.ptr(z), _lib.ptr(d), _lib.ptr(labels), _lib.ptr(regression_targets), R, C, _lib.ptr(n_real),
                                                    _lib.ptr(terms), _lib.ptr(g_z), _lib.ptr(g_d), _lib.ptr(losses), _lib.stream()))
        ctx.grads = (g_z, g_d)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, d_cls, d_box):
        g_z, g_d = ctx.grads
        return g_z * d_cls, g_d * d_box, None, None


def fastrcnn_loss(class_logits, box_regression, labels, regression_targets):
    """fastrcnn_loss of torchvision 0.4.2 over padded rows: class_logits (R,C), box_regression (R,4C) float32, labels (R) int (-1: a padding
    row, neither summed nor counted), regression_targets (R,4).  N = the real rows (background included): loss_classifier = mean(logsumexp(z) -
    z[label]), loss_box_reg = sum over label > 0 of smooth_l1(box_regression[r, 4 label : 4 label + 4] - t[r], beta = 1) / N.
    -> (loss_classifier, loss_box_reg), differentiable with respect to class_logits and box_regression."""
    if not torch.is_tensor(class_logits) or class_logits.dim() != 2:
        raise ValueError(f'class_logits must be (R,C), got {tuple(class_logits.shape) if torch.is_tensor(class_logits) else type(class_logits).__name__}')
    R, C = int(class_logits.shape[0]), int(class_logits.shape[1])
    if R < 1:
        raise ValueError('class_logits must hold at least one row')
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f'{C} classes lie outside [2, {MAX_CLASSES}]')
    detector._tensor(class_logits, 'class_logits', (R, C))
    detector._tensor(box_regression, 'box_regression', (R, 4 * C))
    labels = detector._int_tensor(labels, 'labels', R)
    regression_targets = detector._tensor(regression_targets, 'regression_targets', (R, 4))
    detector._on_device(class_logits=class_logits, box_regression=box_regression, labels=labels, regression_targets=regression_targets)
    return _FastRcnnLossFn.apply(class_logits, box_regression, labels, regression_targets.detach())


# ---- mask targets and loss ---------------------------------------------------------------------------------------------------------------
def _mask_tables(masks, dev):
    ptrs = np.array([m.data_ptr() for m in masks], np.int64)
    dims = np.array([tuple(m.shape) for m in masks], np.int32).reshape(-1, 3)
    return _lib.host_to_device(ptrs, dev), _lib.host_to_device(dims.reshape(-1), dev)


def _mask_side(M):
    M = int(M)
    if not 1 <= M <= MAX_MASK_SIDE:
        raise ValueError(f'M = {M} lies outside [1, {MAX_MASK_SIDE}]')
    return M


def mask_targets(gt_masks, boxes, matched_idxs, M):
    """project_masks_on_boxes for one image: roi_align(gt_masks[:, None], [matched_idx, box], (M, M), spatial_scale 1) with torchvision's
    default sampling_ratio = -1, the ADAPTIVE grid: per axis g = ceil(max(extent, 1) / M) samples per bin.  gt_masks (G,H,W) uint8, read as
    they are; boxes (R,4) float32 (any finite box, inside the frame or not), matched_idxs (R) int.  A row whose matched index lies outside
    [0, G) is written as zeros.  -> (R,M,M) float32 averages, not thresholded."""
    M = _mask_side(M)
    if not torch.is_tensor(gt_masks) or gt_masks.dim() != 3:
        raise ValueError(f'gt_masks must be (G,H,W), got {tuple(gt_masks.shape) if torch.is_tensor(gt_masks) else type(gt_masks).__name__}')
    gt_masks = detector._tensor(gt_masks, 'gt_masks', (None, None, None), torch.uint8)
    if gt_masks.shape[0] < 1 or gt_masks.shape[1] < 1 or gt_masks.shape[2] < 1 or gt_masks.shape[1] * gt_masks.shape[2] >= 1 << 30:
        raise ValueError(f'gt_masks must hold at least one mask of 1 <= H W < 2^30 pixels, got {tuple(gt_masks.shape)}')
    boxes = detector._tensor(boxes, 'boxes', (None, 4))
    R = int(boxes.shape[0])
    matched_idxs = detector._int_tensor(matched_idxs, 'matched_idxs', R)
    detector._on_device(gt_masks=gt_masks, boxes=boxes, matched_idxs=matched_idxs)
    dev = boxes.device
    out = torch.empty((R, M, M), dtype=torch.float32, device=dev)
    if R:
        ptrs, dims = _mask_tables([gt_masks], dev)
        _lib.check(_lib.lib().cosy_dt_mask_loss(_lib.ptr(ptrs), _lib.ptr(dims), 1, _lib.ptr(boxes), None, _lib.ptr(matched_idxs), None, R, None, 1, M, None,
                                                None, _lib.ptr(out), None, _lib.stream()))
    return out


class _MaskLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask_logits, meta):
        masks, B, rows, boxes, labels, matched, pos_counts = meta
        x = mask_logits.detach().contiguous()
        R, C, M = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        dev = x.device
        ptrs, dims = _mask_tables(masks, dev)
        grad = torch.empty_like(x)
        partial = torch.empty(R, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().cosy_dt_mask_loss(_lib.ptr(ptrs), _lib.ptr(dims), B, _lib.ptr(boxes), _lib.ptr(labels), _lib.ptr(matched), _lib.ptr(pos_counts),
                                                rows, _lib.ptr(x), C, M, _lib.ptr(partial), _lib.ptr(grad), None, _lib.ptr(loss), _lib.stream()))
        ctx.grad = grad
        return loss[0]

    @staticmethod
    def backward(ctx, d_loss):
        return ctx.grad * d_loss, None


def maskrcnn_loss(mask_logits, pos_boxes, pos_labels, pos_matched_idxs, targets, pos_counts=None):
    """maskrcnn_loss of torchvision 0.4.2 over padded rows: mask_logits (R,C,M,M) float32, one row per sampled positive RoI, R = B x rows; image
    b owns rows [b rows, (b+1) rows) and its first pos_counts[b] ((B) int32 device tensor; None: all) are real.  pos_boxes (R,4), pos_labels
    (R), pos_matched_idxs (R) int; targets: the images' dicts, whose uint8 masks are read in place (no float copy).  The mask targets are
    mask_targets' (the adaptive grid).  -> loss_mask = mean over (n_pos, M, M) of BCE-with-logits(mask_logits[r, label_r], target_r),
    differentiable with respect to mask_logits; without a positive it is exactly 0 with zero gradients."""
    _, _, masks = _targets(targets, masks=True)
    B = len(masks)
    if not torch.is_tensor(mask_logits) or mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
        raise ValueError(f'mask_logits must be (R,C,M,M), got {tuple(mask_logits.shape) if torch.is_tensor(mask_logits) else type(mask_logits).__name__}')
    R, C, M = int(mask_logits.shape[0]), int(mask_logits.shape[1]), _mask_side(mask_logits.shape[2])
    detector._tensor(mask_logits, 'mask_logits', (R, C, M, M))
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f'{C} classes lie outside [1, {MAX_CLASSES}]')
    if R < 1 or R % B:
        raise ValueError(f'mask_logits hold padded rows, the same number (at least one) for each of the {B} images: got {R} rows')
    if R * C * M * M >= 1 << 31:
        raise ValueError(f'mask_logits of {R} x {C} x {M} x {M} elements exceed the limit of 2^31')
    pos_boxes = detector._tensor(pos_boxes, 'pos_boxes', (R, 4))
    pos_labels = detector._int_tensor(pos_labels, 'pos_labels', R)
    pos_matched_idxs = detector._int_tensor(pos_matched_idxs, 'pos_matched_idxs', R)
    if pos_counts is not None:
        pos_counts = detector._int_tensor(pos_counts, 'pos_counts', B)
    detector._on_device(mask_logits=mask_logits, pos_boxes=pos_boxes, pos_labels=pos_labels, pos_matched_idxs=pos_matched_idxs, masks=masks,
                        pos_counts=pos_counts)
    return _MaskLossFn.apply(mask_logits, (masks, B, R // B, pos_boxes, pos_labels, pos_matched_idxs, pos_counts))


# ---- features -> loss_dict -----------------------------------------------------------------------------------------------------------
def detector_losses(features, rpn_head, box_head, mask_head, targets, net_sizes, padded_size, n_roi_levels=4, keys=None, generator=None,
                    sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS, pre_nms_top_n=2000, post_nms_top_n=2000, rpn_nms_thresh=0.7, min_size=1e-3,
                    box_output_size=7, mask_output_size=14, sampling_ratio=2):
    """The detector's training forward from the FPN's feature maps on: what model(images, targets) returns in training mode.  features and the
    heads as in detector_rpn.detections_from_features; targets: one dict per image (boxes, labels, masks).  keys: None, or a dict with
    'rpn' (B, anchors per image) and 'roi' (B, post_nms_top_n + max G) int32 keys for the two samplers.  Chains rpn_loss, rpn_proposals on the
    DETACHED RPN outputs with torchvision's training values (2000 / 2000), roi_training_samples, multiscale_roi_align(7) + box_head +
    fastrcnn_loss, multiscale_roi_align(14) of the positives + mask_head + maskrcnn_loss.
    -> the reference's loss_dict: loss_objectness, loss_rpn_box_reg, loss_classifier, loss_box_reg, loss_mask: scalars with autograd history
    through the heads and, for feature maps that require grad, through both RoIAligns into the feature maps (cosy_msroi_align_backward), as
    torchvision's Mask R-CNN has it; the proposals carry no gradient.  The heads see padded rows: B x 512 for the box head, B x 128 for the mask head."""
    features = detector_rpn._levels(features, 'features')
    keys = keys or {}
    objectness, deltas = rpn_head(features)
    objectness, deltas = [o.contiguous() for o in objectness], [d.contiguous() for d in deltas]
    loss_objectness, loss_rpn_box_reg = rpn_loss(objectness, deltas, targets, net_sizes, padded_size, sizes, aspect_ratios, keys.get('rpn'), generator)
    proposals, counts, _ = detector_rpn.rpn_proposals([o.detach() for o in objectness], [d.detach() for d in deltas], net_sizes, padded_size, sizes,
                                                      aspect_ratios, pre_nms_top_n, post_nms_top_n, rpn_nms_thresh, min_size)
    smp = roi_training_samples(proposals, counts, targets, keys.get('roi'), generator)
    roi_maps = features[:int(n_roi_levels)]                             # not detached: RoIAlign has a backward into them
    class_logits, box_regression = box_head(detector_rpn.multiscale_roi_align(roi_maps, smp['boxes'], net_sizes, box_output_size, sampling_ratio,
                                                                              counts=smp['counts']))
    loss_classifier, loss_box_reg = fastrcnn_loss(class_logits, box_regression, smp['labels'], smp['regression_targets'])
    mask_logits = mask_head(detector_rpn.multiscale_roi_align(roi_maps, smp['pos_boxes'], net_sizes, mask_output_size, sampling_ratio,
                                                              counts=smp['pos_counts']))
    loss_mask = maskrcnn_loss(mask_logits, smp['pos_boxes'], smp['pos_labels'], smp['pos_matched_idxs'], targets, smp['pos_counts'])
    return dict(loss_objectness=loss_objectness, loss_rpn_box_reg=loss_rpn_box_reg, loss_classifier=loss_classifier, loss_box_reg=loss_box_reg,
                loss_mask=loss_mask)

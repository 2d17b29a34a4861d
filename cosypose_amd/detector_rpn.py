"""Proposal side of the detector: what sits between the trunk's convolutions and the inputs of detector.detections_from_heads.
What torchvision 0.4.2 (AnchorGenerator, RegionProposalNetwork.filter_proposals, MultiScaleRoIAlign) does between the FPN / the RPN head
and the box and mask heads; the convolutions and linears themselves stay ordinary torch.nn modules.  DESIGN.md
section 22 states the contract; HIP: csrc/kernels_detpre.hip; the NMS is detector.py's (cosy_nms_mask / cosy_nms_scan), unchanged.

What runs where
  * device, our kernels: the per-level top-k of the objectness logits (cosy_rpn_select), anchors + decode + clip + small-box test into
    per-image candidate arenas (cosy_rpn_decode), the suppression matrix and the greedy walk (cosy_nms_mask, cosy_nms_scan), the kept rows
    (cosy_rpn_gather), level mapper + RoIAlign of all boxes of all images and levels in one launch (cosy_msroi_align), and its backward
    into the feature maps as a gather without floating-point atomics (cosy_msroi_align_backward);
  * device, torch as plumbing: ONE sort of the candidates' 64-bit keys;
  * host: the base anchors, strides and scales of at most 8 levels (a few dozen numbers).  No device-to-host copy, except the counts for
    rpn_proposals(as_list=True).

Proposals are PADDED rows: image b owns rows [b post_nms_top_n, (b+1) post_nms_top_n) of `proposals`, the first counts[b] of them hold
boxes, the rest zeros.  multiscale_roi_align(counts=<device tensor>) writes zeros for the padding; detector.detections_from_heads decodes a
zero box into a zero box, which its small-box test drops, so the padded rows can be handed on as they are (counts=[post_nms_top_n] * B).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import detector
from .detector import MAX_IMAGES             # the sort key: 11 bits of image, then here 32 of ordered score and 20 of candidate index
from .io_formats import empty_detections

MAX_LEVELS = _lib.RPN_MAX_LEVELS                 # cosy_rpn_levels_t / cosy_msroi_levels_t
MAX_ANCHORS_PER_CELL = _lib.RPN_MAX_ANCHORS
MAX_ANCHORS_PER_IMAGE = 1 << 20
MAX_TAPS = 128                   # output_size * sampling_ratio
DEFAULT_SIZES = ((32,), (64,), (128,), (256,), (512,))
DEFAULT_RATIOS = (0.5, 1.0, 2.0)


# ---- argument checks: all of them run before the library is loaded -----------------------------------------------------------------
def _feature(t, name, shape):
    """a head output or a feature map: read in place, so it must be what the kernels index -- float32, contiguous, of the shape"""
    if not torch.is_tensor(t):
        raise ValueError(f'{name} must be a tensor, got {type(t).__name__}')
    if t.dim() != len(shape) or any(s is not None and int(e) != s for e, s in zip(t.shape, shape)):
        want = '(' + ','.join('*' if s is None else str(s) for s in shape) + ')'
        raise ValueError(f'{name} must be {want}, got {tuple(t.shape)}')
    if t.dtype != torch.float32:
        raise ValueError(f'{name} must be torch.float32, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous (NCHW): it is read in place')
    return t


def _levels(maps, name):
    if torch.is_tensor(maps) or not isinstance(maps, (list, tuple)):
        raise ValueError(f'{name} must be a list of one tensor per level, got {type(maps).__name__}')
    if not 1 <= len(maps) <= MAX_LEVELS:
        raise ValueError(f'{name} must hold 1 to {MAX_LEVELS} levels, got {len(maps)}')
    return list(maps)


def _pair(v, name):
    h, w = (int(x) for x in v)
    if h < 1 or w < 1:
        raise ValueError(f'{name} must be a positive (height, width), got {(h, w)}')
    return h, w


def base_anchors(sizes, aspect_ratios):
    """AnchorGenerator.generate_anchors for one level in float32: (len(aspect_ratios) * len(sizes), 4), ratio-major, rounded half to even"""
    scales, ar = np.asarray(sizes, np.float32).reshape(-1), np.asarray(aspect_ratios, np.float32).reshape(-1)
    if scales.size == 0 or ar.size == 0 or not (scales > 0).all() or not (ar > 0).all():
        raise ValueError(f'anchor sizes and aspect ratios must be positive, got {sizes}, {aspect_ratios}')
    h_r = np.sqrt(ar)
    w_r = np.float32(1) / h_r
    ws, hs = (w_r[:, None] * scales[None, :]).reshape(-1), (h_r[:, None] * scales[None, :]).reshape(-1)
    return np.round(np.stack([-ws, -hs, ws, hs], 1) / np.float32(2)).astype(np.float32)


def _anchor_tables(feature_sizes, padded_size, sizes, aspect_ratios):
    """-> [(H, W, stride_h, stride_w, base (A,4))] per level, A; every limit of the kernels' index fields is refused here, by name"""
    pad_h, pad_w = _pair(padded_size, 'padded_size')
    L = len(feature_sizes)
    if len(sizes) != L:
        raise ValueError(f'sizes must hold one tuple of anchor sizes per level: {L} levels, got {len(sizes)}')
    out, total = [], 0
    for l, (fs, sz) in enumerate(zip(feature_sizes, sizes)):
        H, W = _pair(fs, f'feature_sizes[{l}]')
        base = base_anchors(sz, aspect_ratios)
        out.append((H, W, np.float32(pad_h / H), np.float32(pad_w / W), base))
        total += base.shape[0] * H * W
    A = out[0][4].shape[0]
    if any(t[4].shape[0] != A for t in out):
        raise ValueError(f'every level must have the same number of anchors per cell, got {[t[4].shape[0] for t in out]}')
    if A > MAX_ANCHORS_PER_CELL:
        raise ValueError(f'{A} anchors per cell exceed the limit of {MAX_ANCHORS_PER_CELL}')
    if total > MAX_ANCHORS_PER_IMAGE:
        raise ValueError(f'{total} anchors per image exceed the limit of 2^20 = {MAX_ANCHORS_PER_IMAGE} (the candidate index field of the sort key)')
    return out, A


def rpn_anchors(feature_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS):
    """AnchorGenerator's table for one image: feature_sizes [(H_l, W_l)], padded_size (height, width) of the batch -> (sum A H_l W_l, 4)
    float32 CPU tensor, row = the candidate index the kernels use: level offset + (y W_l + x) A + a.  The kernels never read this table:
    they form an anchor from its index."""
    tables, A = _anchor_tables(list(feature_sizes), padded_size, sizes, aspect_ratios)
    rows = []
    for H, W, sh, sw, base in tables:
        sx, sy = np.arange(W, dtype=np.float32) * sw, np.arange(H, dtype=np.float32) * sh
        shift = np.stack([np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W))] * 2, -1).reshape(H * W, 1, 4)
        rows.append((shift + base[None]).reshape(-1, 4))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32))


class AnchorGrid:
    """the anchors of one image as the kernels form them from an index: section 22 step 1's level description, no table; fills every RpnLevels"""

    def __init__(self, feature_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS):
        feature_sizes = [tuple(int(v) for v in s) for s in feature_sizes]
        if not 1 <= len(feature_sizes) <= MAX_LEVELS:
            raise ValueError(f'feature_sizes must hold 1 to {MAX_LEVELS} levels, got {len(feature_sizes)}')
        self.tables, self.A = _anchor_tables(feature_sizes, padded_size, sizes, aspect_ratios)
        self.L = len(feature_sizes)
        self.N = sum(self.A * H * W for H, W, *_ in self.tables)

    @classmethod
    def cells(cls, objectness):
        """the cells of the head's outputs alone, for a launch that forms no anchor (rpn_select): strides and base anchors stay zero"""
        grid = cls.__new__(cls)
        grid.tables = [(int(o.shape[2]), int(o.shape[3]), 0.0, 0.0, np.zeros((0, 4), np.float32)) for o in objectness]
        grid.A, grid.L = int(objectness[0].shape[1]), len(objectness)
        return grid

    def levels(self, objectness=None, deltas=None):
        lv = _lib.RpnLevels()
        for l, (H, W, sh, sw, base) in enumerate(self.tables):
            lv.H[l], lv.W[l], lv.stride_h[l], lv.stride_w[l] = H, W, float(sh), float(sw)
            if objectness is not None:
                lv.objectness[l], lv.deltas[l] = objectness[l].data_ptr(), deltas[l].data_ptr()
            for a in range(base.shape[0]):
                for c in range(4):
                    lv.base[l][a][c] = float(base[a, c])
        return lv


def _rpn_heads(objectness, bbox_deltas):
    """the RPN head's outputs, one (B,A,H_l,W_l) / (B,4A,H_l,W_l) pair per level, read in place -> objectness, bbox_deltas (lists), B, A, L"""
    objectness, bbox_deltas = _levels(objectness, 'objectness'), _levels(bbox_deltas, 'bbox_deltas')
    L = len(objectness)
    if len(bbox_deltas) != L:
        raise ValueError(f'objectness holds {L} levels, bbox_deltas {len(bbox_deltas)}')
    if not torch.is_tensor(objectness[0]) or objectness[0].dim() != 4:
        raise ValueError(f'objectness[0] must be (B,A,H,W), got {tuple(objectness[0].shape) if torch.is_tensor(objectness[0]) else type(objectness[0]).__name__}')
    B, A = int(objectness[0].shape[0]), int(objectness[0].shape[1])
    for l in range(L):
        o = _feature(objectness[l], f'objectness[{l}]', (B, A, None, None))
        _feature(bbox_deltas[l], f'bbox_deltas[{l}]', (B, 4 * A, int(o.shape[2]), int(o.shape[3])))
    return objectness, bbox_deltas, B, A, L


def _rpn_grid(objectness, A, padded_size, sizes, aspect_ratios):
    grid = AnchorGrid([tuple(o.shape[2:]) for o in objectness], padded_size, sizes, aspect_ratios)
    if grid.A != A:
        raise ValueError(f'objectness has {A} anchors per cell, sizes x aspect_ratios give {grid.A}')
    return grid


def rpn_proposals(objectness, bbox_deltas, net_sizes, padded_size, sizes=DEFAULT_SIZES, aspect_ratios=DEFAULT_RATIOS, pre_nms_top_n=1000,
                  post_nms_top_n=1000, nms_thresh=0.7, min_size=1e-3, as_list=False, return_source=False):
    """RegionProposalNetwork.filter_proposals (inference) over the RPN head's raw outputs, all images and levels at once.
    objectness[l] (B,A,H_l,W_l), bbox_deltas[l] (B,4A,H_l,W_l): float32, contiguous, on the device, read in place; net_sizes: (height,
    width) of every image as the network saw it (the clip); padded_size: of the batch (the strides).
    -> proposals (B post_nms_top_n, 4) float32, counts (B) int32, scores (B post_nms_top_n) float32 on the device: image b owns the rows
    [b post_nms_top_n, (b+1) post_nms_top_n), the first counts[b] of them by descending objectness LOGIT (no sigmoid: torchvision 0.4.2),
    the rest zeros[, with return_source also levels and candidate indices (int32, -1 on padding)].  as_list: the list of (counts[b], 4)
    tensors instead (one small device-to-host copy).  Equal logits: lower candidate index first, at the k-th place too; an anchor whose
    logit or any delta is NaN is absent."""
    objectness, bbox_deltas, B, A, L = _rpn_heads(objectness, bbox_deltas)
    grid = _rpn_grid(objectness, A, padded_size, sizes, aspect_ratios)
    pre, post = int(pre_nms_top_n), int(post_nms_top_n)
    if pre < 1 or post < 1:
        raise ValueError(f'pre_nms_top_n and post_nms_top_n must be positive, got {pre}, {post}')
    if (pre * L + 63) // 64 * 64 > detector.MAX_CANDIDATES:
        raise ValueError(f'pre_nms_top_n x levels = {pre} x {L} = {pre * L}, rounded up to 64, exceeds cosy_nms_max_candidates() = '
                         f'{detector.MAX_CANDIDATES} candidates per image')
    cap = max(64, (pre * L + 63) // 64 * 64)
    if B > MAX_IMAGES:
        raise ValueError(f'{B} images exceed the limit of {MAX_IMAGES} per call')
    if not 0 <= float(min_size):
        raise ValueError(f'min_size must not be negative, got {min_size}')
    net = detector._sizes(net_sizes, 'net_sizes', B)
    pad_h, pad_w = _pair(padded_size, 'padded_size')
    if B and ((net[:, 0] > pad_h).any() or (net[:, 1] > pad_w).any()):
        raise ValueError(f'net_sizes {net.tolist()} exceed padded_size {(pad_h, pad_w)}')
    detector._on_device(objectness=objectness, bbox_deltas=bbox_deltas)
    dev = objectness[0].device
    if B == 0:
        out = (torch.empty((0, 4), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
               torch.empty(0, dtype=torch.float32, device=dev))
        if as_list:
            return []
        return out + (torch.empty(0, dtype=torch.int32, device=dev),) * 2 if return_source else out
    lv = grid.levels(objectness, bbox_deltas)
    net_dev = _lib.host_to_device(net.astype(np.float32).reshape(-1), dev)
    sel_idx = torch.empty((B, L, pre), dtype=torch.int32, device=dev)
    sel_count = torch.empty((B, L), dtype=torch.int32, device=dev)
    arena = detector._arena(B, cap, dev)                                 # (its labels: the candidates' levels)
    l_ = _lib.lib()
    _lib.check(l_.cosy_rpn_select(ctypes.byref(lv), L, A, B, pre, _lib.ptr(sel_idx), _lib.ptr(sel_count), _lib.stream()))
    _lib.check(l_.cosy_rpn_decode(ctypes.byref(lv), L, A, B, pre, _lib.ptr(sel_idx), _lib.ptr(sel_count), _lib.ptr(net_dev), float(min_size), cap,
                                  *map(_lib.ptr, arena), _lib.stream()))
    kept, n_kept = detector._arena_nms(arena, B, cap, nms_thresh, post)
    proposals = torch.empty((B * post, 4), dtype=torch.float32, device=dev)
    scores = torch.empty(B * post, dtype=torch.float32, device=dev)
    levels = torch.empty(B * post, dtype=torch.int32, device=dev)
    src = torch.empty(B * post, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(l_.cosy_rpn_gather(_lib.ptr(kept), _lib.ptr(n_kept), *map(_lib.ptr, arena[:4]), B, cap, post, _lib.ptr(proposals), _lib.ptr(scores), _lib.ptr(levels), _lib.ptr(src), _lib.ptr(counts), _lib.stream()))
    if as_list:
        host = counts.cpu().tolist()                                       # THE device-to-host copy of the list form
        return [proposals[b * post:b * post + n] for b, n in enumerate(host)]
    return (proposals, counts, scores, levels, src) if return_source else (proposals, counts, scores)


def rpn_select(objectness, bbox_deltas, pre_nms_top_n):
    """the first launch of rpn_proposals on its own: -> sel_idx (B,L,pre_nms_top_n) int32, sel_count (B,L) int32 on the device; the first
    sel_count[b,l] entries of sel_idx[b,l] are the anchors of level l taken for image b: those strictly above the k-th logit in ascending
    index order, then the lowest-index anchors at it.  Rows past sel_count are not written."""
    objectness, bbox_deltas, B, A, L = _rpn_heads(objectness, bbox_deltas)
    pre = int(pre_nms_top_n)
    if pre < 1 or pre * L > detector.MAX_CANDIDATES:
        raise ValueError(f'pre_nms_top_n x levels = {pre} x {L} must lie in [1, cosy_nms_max_candidates() = {detector.MAX_CANDIDATES}]')
    detector._on_device(objectness=objectness, bbox_deltas=bbox_deltas)
    dev = objectness[0].device
    lv = AnchorGrid.cells(objectness).levels(objectness, bbox_deltas)
    sel_idx = torch.full((B, L, pre), -1, dtype=torch.int32, device=dev)
    sel_count = torch.zeros((B, L), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().cosy_rpn_select(ctypes.byref(lv), L, A, B, pre, _lib.ptr(sel_idx), _lib.ptr(sel_count), _lib.stream()))
    return sel_idx, sel_count


# ---- MultiScaleRoIAlign --------------------------------------------------------------------------------------------------------------
def infer_scales(feature_sizes, net_sizes):
    """MultiScaleRoIAlign.setup_scales: scales[l] = 2^round(log2(H_l / max image height)), checked equal to the same from the widths"""
    net = np.asarray(net_sizes, np.int64).reshape(-1, 2)
    if net.shape[0] == 0:
        raise ValueError('scales cannot be inferred without an image: pass net_sizes or scales')
    max_h, max_w = int(net[:, 0].max()), int(net[:, 1].max())
    scales = []
    for l, (H, W) in enumerate(feature_sizes):
        s_h = 2.0 ** float(np.round(np.log2(np.float32(float(H) / float(max_h)))))
        s_w = 2.0 ** float(np.round(np.log2(np.float32(float(W) / float(max_w)))))
        if s_h != s_w:
            raise ValueError(f'level {l}: the scale from the heights ({H} / {max_h} -> {s_h}) differs from the scale from the widths ({W} / {max_w} -> {s_w})')
        scales.append(s_h)
    return scales


def multiscale_roi_align(features, boxes, net_sizes, output_size, sampling_ratio=2, batch_im_id=None, counts=None, scales=None,
                         return_levels=False):
    """MultiScaleRoIAlign: features[l] (B,C,H_l,W_l) float32, contiguous, on the device; boxes (R,4) xyxy float32 at the network's scale,
    or a list of (R_i,4), one per image.  The image of a row comes from exactly one of
      batch_im_id (R) int tensor;
      counts: a list of B ints summing to R (image by image), or a (B) int32 DEVICE tensor for padded rows -- R = B x rows, image b owns
        rows [b rows, (b+1) rows) and only its first counts[b] are boxes; the rest are written as zeros (rpn_proposals' layout);
      the list form of boxes.
    scales: spatial scale of every level; None: inferred from net_sizes as torchvision does.  Level = clamp(floor(4 + log2(sqrt(area) / 224
    + 1e-6)), k_min, k_max) - k_min with k = -log2(scale) of the first and last level, rounded to an integer.
    -> (R,C,P,P) float32[, levels (R) int32] on the device, P = output_size.  With autograd enabled and a feature map that requires grad the
    result carries a backward into those feature maps (none into the boxes); otherwise the code path is the plain launch."""
    features = _levels(features, 'features')
    L = len(features)
    if not torch.is_tensor(features[0]) or features[0].dim() != 4:
        raise ValueError(f'features[0] must be (B,C,H,W), got {tuple(features[0].shape) if torch.is_tensor(features[0]) else type(features[0]).__name__}')
    B, C = int(features[0].shape[0]), int(features[0].shape[1])
    for l in range(L):
        _feature(features[l], f'features[{l}]', (B, C, None, None))
    if C < 1 or any(f.shape[2] < 1 or f.shape[3] < 1 for f in features):
        raise ValueError(f'features must have at least one channel and one cell, got {[tuple(f.shape) for f in features]}')
    P, g = int(output_size), int(sampling_ratio)
    if g <= 0:
        raise ValueError(f'sampling_ratio must be > 0, got {sampling_ratio} (the adaptive grid of sampling_ratio <= 0 is not implemented)')
    if P < 1 or P * g > MAX_TAPS:
        raise ValueError(f'output_size x sampling_ratio = {P} x {g} must lie in [1, {MAX_TAPS}]')
    im_id = rows = dev_counts = None
    if not torch.is_tensor(boxes):
        parts = [detector._tensor(b, f'boxes[{i}]', (None, 4)) for i, b in enumerate(boxes)]
        if batch_im_id is not None or counts is not None:
            raise ValueError('boxes given as a list name their images themselves: no batch_im_id, no counts')
        counts = [int(p.shape[0]) for p in parts]
    else:
        boxes = detector._tensor(boxes, 'boxes', (None, 4))
        parts = None
        if (batch_im_id is None) == (counts is None):
            raise ValueError('boxes given as one (R,4) tensor need exactly one of batch_im_id and counts')
    R = int(sum(p.shape[0] for p in parts)) if parts is not None else int(boxes.shape[0])
    if batch_im_id is not None:
        im_id = detector._int_tensor(batch_im_id, 'batch_im_id', R)
    elif torch.is_tensor(counts):
        dev_counts = detector._int_tensor(counts, 'counts', B)
        if B == 0 or R % B:
            raise ValueError(f'counts as a tensor go with padded rows, the same number for each of the {B} images: got {R} rows')
        rows = R // B
    else:
        counts = [int(c) for c in counts]
        if len(counts) != B or any(c < 0 for c in counts) or sum(counts) != R:
            raise ValueError(f'counts must hold one non-negative number per image ({B}) summing to {R} rows, got {counts}')
    if scales is None:
        scales = infer_scales([tuple(int(v) for v in f.shape[2:]) for f in features], detector._sizes(net_sizes, 'net_sizes', B))
    scales = [float(s) for s in scales]
    if len(scales) != L or any(not s > 0 for s in scales):
        raise ValueError(f'scales must hold one positive number per level ({L}), got {scales}')
    k_min, k_max = int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1])))
    if not 0 <= k_max - k_min < L:
        raise ValueError(f'scales {scales} give k_min = {k_min}, k_max = {k_max}, which do not index {L} levels')
    detector._on_device(features=features, boxes=parts if parts is not None else boxes, batch_im_id=im_id, counts=dev_counts)
    dev = features[0].device
    if parts is not None:
        boxes = torch.cat(parts) if parts else torch.empty((0, 4), dtype=torch.float32, device=dev)
    if R and im_id is None and rows is None:
        im_id = _lib.ints_to_device(np.repeat(np.arange(B), counts), dev)
    call = dict(L=L, B=B, C=C, R=R, P=P, g=g, k_min=k_min, k_max=k_max, rows=rows or 0, scales=scales, boxes=boxes, im_id=im_id, counts=dev_counts,
                return_levels=return_levels)
    if torch.is_grad_enabled() and any(f.requires_grad for f in features):
        out, levels = _MsroiAlignFn.apply(call, *features)          # the same launch, with a backward into the feature maps
    else:
        out, levels = _msroi_forward(call, features)
    return (out, levels) if return_levels else out


def _msroi_table(call, maps):
    lv = _lib.MsroiLevels()
    for l, (H, W) in enumerate(maps):
        lv.H[l], lv.W[l], lv.scale[l] = H, W, call['scales'][l]
    return lv


def _msroi_forward(call, features):
    R, C, P = call['R'], call['C'], call['P']
    dev = features[0].device
    out = torch.empty((R, C, P, P), dtype=torch.float32, device=dev)
    levels = torch.empty(R, dtype=torch.int32, device=dev) if call['return_levels'] else None
    if R:
        lv = _msroi_table(call, [f.shape[2:] for f in features])
        for l, f in enumerate(features):
            lv.feat[l] = f.data_ptr()
        _lib.check(_lib.lib().cosy_msroi_align(ctypes.byref(lv), call['L'], call['B'], C, _lib.ptr(call['boxes']), _lib.ptr(call['im_id']),
                                               _lib.ptr(call['counts']), call['rows'], R, P, call['g'], call['k_min'], call['k_max'], _lib.ptr(out),
                                               _lib.ptr(levels), _lib.stream()))
    return out, levels


class _MsroiAlignFn(torch.autograd.Function):
    """multiscale_roi_align with a gradient for the feature maps (cosy_msroi_align_backward); none for the boxes"""

    @staticmethod
    def forward(ctx, call, *features):
        out, levels = _msroi_forward(call, [f.detach() for f in features])
        ctx.call, ctx.maps = call, [tuple(int(v) for v in f.shape[2:]) for f in features]
        if levels is not None:
            ctx.mark_non_differentiable(levels)
        return out, levels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_levels=None):
        call, L = ctx.call, ctx.call['L']
        grad_out = grad_out.to(torch.float32).contiguous()
        dev = grad_out.device
        grads = [torch.empty((call['B'], call['C'], H, W), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1 + l] else None
                 for l, (H, W) in enumerate(ctx.maps)]
        ptrs = (ctypes.c_void_p * _lib.RPN_MAX_LEVELS)(*[_lib.ptr(t) for t in grads])
        ws = torch.empty(8 * call['R'], dtype=torch.int32, device=dev)
        lv = _msroi_table(call, ctx.maps)
        _lib.check(_lib.lib().cosy_msroi_align_backward(ctypes.byref(lv), ptrs, L, call['B'], call['C'], _lib.ptr(grad_out), _lib.ptr(call['boxes']),
                                                        _lib.ptr(call['im_id']), _lib.ptr(call['counts']), call['rows'], call['R'], call['P'],
                                                        call['g'], call['k_min'], call['k_max'], _lib.ptr(ws), _lib.stream()))
        return (None, *grads)


def roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=2):
    """torchvision.ops.roi_align (0.4.2: no `aligned`) of one feature map: input (B,C,H,W) float32, contiguous, on the device; boxes (K,5)
    float32 with the image index in column 0, or a list of (K_i,4), one per image.  multiscale_roi_align with one level, so differentiable
    with respect to input; sampling_ratio <= 0 (the adaptive grid) is refused.  -> (K,C,P,P), P = output_size."""
    if torch.is_tensor(boxes):
        boxes = detector._tensor(boxes, 'boxes', (None, 5))
        return multiscale_roi_align([input], boxes[:, 1:].contiguous(), None, output_size, sampling_ratio, batch_im_id=boxes[:, 0].to(torch.int32),
                                    scales=[spatial_scale])
    return multiscale_roi_align([input], boxes, None, output_size, sampling_ratio, scales=[spatial_scale])


# ---- features -> detections ----------------------------------------------------------------------------------------------------------
RPN_OPTIONS = ('sizes', 'aspect_ratios', 'pre_nms_top_n', 'post_nms_top_n', 'min_size')


def detections_from_features(features, rpn_head, box_head, mask_head, net_sizes, padded_size, original_sizes, category_id_to_label,
                             rpn_nms_thresh=0.7, n_roi_levels=4, box_output_size=7, mask_output_size=14, sampling_ratio=2, **filters):
    """The detector from the FPN's feature maps on.  features: list of (B,C,H_l,W_l), every level the RPN sees (Mask R-CNN: '0'..'3' and
    'pool'); the first n_roi_levels of them feed RoIAlign (Mask R-CNN: 4).  The heads are ordinary torch.nn modules or callables:
      rpn_head(features) -> (objectness, bbox_deltas), lists with one (B,A,H_l,W_l) / (B,4A,H_l,W_l) tensor per level;
      box_head(roi_feats (R,C,7,7)) -> (class_logits (R,K), box_regression (R,4K));
      mask_head(roi_feats (D,C,14,14)) -> (D,K,M,M), called once, on the detections that survive the filters; None without masks.
    Chains rpn_proposals, multiscale_roi_align(7), box_head and detector.detections_from_heads, whose mask callable is
    multiscale_roi_align(14) followed by mask_head.  `filters`: rpn_proposals' sizes, aspect_ratios, pre_nms_top_n, post_nms_top_n,
    min_size, and every option of detections_from_heads (detection_th, one_instance_per_class, output_masks, mask_th, score_thresh,
    nms_thresh, detections_per_img, max_candidates).  The box head sees all B x post_nms_top_n padded rows (a padding row: zero features,
    a zero box, dropped by the small-box test), so nothing is copied to the host before detections_from_heads' own copy."""
    features = _levels(features, 'features')
    rpn_kw = {k: filters.pop(k) for k in RPN_OPTIONS if k in filters}
    B = int(features[0].shape[0]) if torch.is_tensor(features[0]) and features[0].dim() == 4 else -1
    if B == 0:
        return empty_detections(features[0].device)
    roi_maps = features[:int(n_roi_levels)]
    objectness, deltas = rpn_head(features)
    objectness, deltas = [o.contiguous() for o in objectness], [d.contiguous() for d in deltas]
    proposals, counts, _ = rpn_proposals(objectness, deltas, net_sizes, padded_size, nms_thresh=rpn_nms_thresh, **rpn_kw)
    post = proposals.shape[0] // B
    class_logits, box_regression = box_head(multiscale_roi_align(roi_maps, proposals, net_sizes, box_output_size, sampling_ratio, counts=counts))

    def masks_of(boxes_net, im_ids):
        return mask_head(multiscale_roi_align(roi_maps, boxes_net, net_sizes, mask_output_size, sampling_ratio, batch_im_id=im_ids))
    return detector.detections_from_heads(class_logits, box_regression, proposals, net_sizes, original_sizes,
                                          category_id_to_label, mask_head=masks_of if filters.get('output_masks') else None,
                                          counts=[post] * B, **filters)

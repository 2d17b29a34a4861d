"""Output side of the detector: from the Mask R-CNN heads' raw outputs to the `detections` collection CoarseRefinePosePredictor takes.
What torchvision 0.4.2 (roi_heads.postprocess_detections, ops.batched_nms, GeneralizedRCNNTransform.postprocess, maskrcnn_inference,
paste_masks_in_image) and Detector.get_detections (cosypose/integrated/detector.py:28-50) do after the network; the network's
convolutions stay out of scope.  DESIGN.md section 21 states the contract; HIP: csrc/kernels_detpost.hip.

What runs where
  * device, our kernels: softmax + box decode + clip + thresholds into per-image candidate arenas (cosy_det_decode), the suppression
    matrix and the greedy walk over it (cosy_nms_mask, cosy_nms_scan), the kept rows and their frame-scale boxes (cosy_det_gather),
    the bool masks (cosy_paste_masks);
  * device, torch as plumbing: ONE sort of the candidates' 64-bit keys, index_select of the rows the host filters chose;
  * host: ONE device-to-host copy (candidate counts, kept counts, labels, scores of at most B x detections_per_img rows), the
    `detection_th` / `one_instance_per_class` filters on those few numbers, the pandas table.

Candidates per image are capped at `max_candidates` (default 4096, at most MAX_CANDIDATES = 16384: the suppression matrix takes
cap^2 / 8 bytes per image); an image with more is REFUSED with a ValueError, never truncated.  Equal scores are visited lower candidate
index first (candidate index = proposal * (C-1) + label - 1; for nms / batched_nms the box's own index).
"""
import collections

import numpy as np
import pandas as pd
import torch

from . import _lib
from . import tensor_collection as tc
from .io_formats import empty_detections

MAX_CANDIDATES = 16384          # cosy_nms_max_candidates()
DEFAULT_CANDIDATES = 4096
MAX_MASK_SIDE = 62
MAX_IMAGES = 2047               # ARENA_MAX_IMAGES: 11 bits of image in the sort key, for every side of the detector (detector_rpn, detector_train)
MAX_CLASSES = _lib.DT_MAX_CLASSES       # cosy_det_decode's limit too
MAX_CANDIDATE_INDEX = 1 << 21   # cosy_det_decode's 21 bits of candidate index in the sort key


# ---- argument checks: all of them run before the library is loaded -----------------------------------------------------------------
def _tensor(t, name, shape, dtype=torch.float32):
    """shape: tuple with None for a free extent"""
    if not torch.is_tensor(t):
        raise ValueError(f'{name} must be a tensor, got {type(t).__name__}')
    if t.dim() != len(shape) or any(s is not None and int(e) != s for e, s in zip(t.shape, shape)):
        want = '(' + ','.join('*' if s is None else str(s) for s in shape) + ')'
        raise ValueError(f'{name} must be {want}, got {tuple(t.shape)}')
    if t.dtype != dtype:
        raise ValueError(f'{name} must be {dtype}, got {t.dtype}')
    return t.contiguous()


def _int_tensor(t, name, n):
    if not torch.is_tensor(t):
        raise ValueError(f'{name} must be a tensor, got {type(t).__name__}')
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f'{name} must be ({n}), got {tuple(t.shape)}')
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'{name} must be int32 or int64, got {t.dtype}')
    return t.to(torch.int32).contiguous()


def _on_device(**tensors):
    """after every shape and dtype check, before anything touches the library"""
    for name, t in tensors.items():
        for i, one in enumerate(t if isinstance(t, (list, tuple)) else [t]):
            if one is not None and not one.is_cuda:
                which = f'{name}[{i}]' if isinstance(t, (list, tuple)) else name
                raise ValueError(f'{which} must live on the ROCm device (got a CPU tensor); there is no CPU fallback')
    _lib.require_device(*[one for t in tensors.values() for one in (t if isinstance(t, (list, tuple)) else [t])])


def _sizes(sizes, name, B):
    arr = np.asarray([tuple(int(v) for v in s) for s in sizes], dtype=np.int64).reshape(-1, 2) if len(sizes) else np.zeros((0, 2), np.int64)
    if arr.shape[0] != B:
        raise ValueError(f'{name} must hold one (height, width) per image: {B} images, got {arr.shape[0]}')
    if (arr < 1).any():
        raise ValueError(f'{name} must be positive, got {arr.tolist()}')
    return arr


def _cap(n, what):
    if n > MAX_CANDIDATES:
        raise ValueError(f'{what}: {n} boxes exceed the cap of {MAX_CANDIDATES} per call (the suppression matrix takes n^2 / 8 bytes)')
    return max(64, (n + 63) // 64 * 64)


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
def _nms_segments(boxes, order, labels, max_coord, seg_start, seg_count, B, cap, iou_threshold, max_keep, flags=False):
    """the two launches -> kept (B, max_keep) int32, n_kept (B) int32[, keep flags (N) uint8] on the device"""
    N, dev = boxes.shape[0], boxes.device
    mask = torch.empty(B * cap * (cap // 64), dtype=torch.int64, device=dev)
    kept = torch.empty((B, max_keep), dtype=torch.int32, device=dev)
    n_kept = torch.empty(B, dtype=torch.int32, device=dev)
    keep_flags = torch.empty(N, dtype=torch.uint8, device=dev) if flags else None
    l = _lib.lib()
    _lib.check(l.cosy_nms_mask(_lib.ptr(boxes), _lib.ptr(order), _lib.ptr(labels), _lib.ptr(max_coord), _lib.ptr(seg_start), _lib.ptr(seg_count),
                               B, N, cap, float(iou_threshold), _lib.ptr(mask), _lib.stream()))
    _lib.check(l.cosy_nms_scan(_lib.ptr(mask), _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(seg_count), B, N, cap, max_keep,
                               _lib.ptr(kept), _lib.ptr(n_kept), _lib.ptr(keep_flags), _lib.stream()))
    return (kept, n_kept, keep_flags) if flags else (kept, n_kept)


_Arena = collections.namedtuple('_Arena', 'boxes scores labels src keys counts max_coord')


def _arena(B, cap, dev):
    """the candidate arena of B images x cap slots (csrc/det_device.h), in the order both decode entry points take it; labels: what NMS keeps apart"""
    n, f32, i32 = B * cap, torch.float32, torch.int32
    layout = (((n, 4), f32), (n, f32), (n, i32), (n, i32), (n, torch.int64), (B, i32), (B, f32))
    return _Arena(*[torch.empty(shape, dtype=kind, device=dev) for shape, kind in layout])


def _arena_nms(arena, B, cap, iou_threshold, max_keep):
    """after the caller's decode launch: ONE sort of the keys (unique: image, score descending, candidate index), then NMS image by image"""
    order = torch.sort(arena.keys)[1]
    seg_start = _lib.ints_to_device(np.arange(B) * cap, arena.keys.device)
    return _nms_segments(arena.boxes, order, arena.labels, arena.max_coord, seg_start, arena.counts, B, cap, iou_threshold, max_keep)


def _nms(boxes, scores, idxs, iou_threshold, what):
    boxes = _tensor(boxes, 'boxes', (None, 4))
    N = boxes.shape[0]
    scores = _tensor(scores, 'scores', (N,))
    labels = None if idxs is None else _int_tensor(idxs, 'idxs', N)
    cap = _cap(N, what)
    _on_device(boxes=boxes, scores=scores, idxs=labels)
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]            # equal scores: the lower index first
    max_coord = None if labels is None else boxes.max().reshape(1)
    seg = _lib.ints_to_device([0, N], boxes.device)
    kept, n_kept = _nms_segments(boxes, order, labels, max_coord, seg[:1], seg[1:], 1, cap, iou_threshold, N)
    return kept[0, :int(n_kept.item())].long()


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: boxes (N,4) xyxy float32, scores (N) float32 -> int64 indices of the kept boxes by descending score.  A box
    is dropped when its IoU (box_iou's float32 arithmetic) with a kept, better box is strictly greater than the threshold; equal
    scores are visited lower index first.  At most MAX_CANDIDATES boxes."""
    return _nms(boxes, scores, None, iou_threshold, 'nms')


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.batched_nms: NMS among the boxes of one category only.  As torchvision does it, every box is shifted by
    float(idx) * (boxes.max() + 1) in float32 before the IoU, so boxes of different categories never overlap."""
    return _nms(boxes, scores, idxs, iou_threshold, 'batched_nms')


# ---- heads -> detections -----------------------------------------------------------------------------------------------------------
def _proposals(proposals, counts):
    if torch.is_tensor(proposals):
        if counts is None:
            raise ValueError('proposals given as one (R,4) tensor need `counts`, the number of proposals of every image')
        counts = [int(c) for c in counts]
        props = _tensor(proposals, 'proposals', (None, 4))
    else:
        proposals = list(proposals)
        if counts is not None:
            raise ValueError('`counts` goes with proposals given as one (R,4) tensor, not with a list')
        checked = [_tensor(p, f'proposals[{i}]', (None, 4)) for i, p in enumerate(proposals)]
        counts = [int(p.shape[0]) for p in checked]
        props = checked
    if any(c < 0 for c in counts):
        raise ValueError(f'counts must not be negative, got {counts}')
    return props, counts


class _Padded:
    """what the launches leave on the device: B x detections_per_img padded rows and the int32 block the host reads"""


def _run(class_logits, box_regression, proposals, net_sizes, original_sizes, counts, score_thresh, nms_thresh, detections_per_img,
         max_candidates):
    props, counts = _proposals(proposals, counts)
    B, R = len(counts), int(sum(counts))
    if not torch.is_tensor(class_logits) or class_logits.dim() != 2:
        raise ValueError(f'class_logits must be (R,C), got {tuple(class_logits.shape) if torch.is_tensor(class_logits) else type(class_logits).__name__}')
    C = int(class_logits.shape[1])
    if C < 2:
        raise ValueError(f'class_logits must have a background column and at least one class, got C = {C}')
    # the sort key's fields (image << 52 | score << 21 | candidate index): refused here, by name, before anything is allocated or launched
    if B > MAX_IMAGES:
        raise ValueError(f'{B} images exceed the limit of {MAX_IMAGES} per call')
    if C > MAX_CLASSES:
        raise ValueError(f'C = {C} classes exceed the limit of {MAX_CLASSES}')
    if R * (C - 1) > MAX_CANDIDATE_INDEX:
        raise ValueError(f'R (C-1) = {R} x {C - 1} = {R * (C - 1)} exceeds the limit of 2^21 = {MAX_CANDIDATE_INDEX} candidate indices per call')
    class_logits = _tensor(class_logits, 'class_logits', (R, C))
    box_regression = _tensor(box_regression, 'box_regression', (R, 4 * C))
    if torch.is_tensor(props) and props.shape[0] != R:
        raise ValueError(f'proposals hold {props.shape[0]} rows, counts sum to {R}')
    net = _sizes(net_sizes, 'net_sizes', B)
    orig = net if original_sizes is None else _sizes(original_sizes, 'original_sizes', B)
    cap, dpi = int(max_candidates), int(detections_per_img)
    if cap < 64 or cap > MAX_CANDIDATES or cap % 64:
        raise ValueError(f'max_candidates must be a multiple of 64 in [64, {MAX_CANDIDATES}], got {cap}')
    if dpi < 1:
        raise ValueError(f'detections_per_img must be positive, got {dpi}')
    if not 0 <= float(score_thresh):
        raise ValueError(f'score_thresh must not be negative, got {score_thresh}')
    _on_device(class_logits=class_logits, box_regression=box_regression, proposals=props)
    if not torch.is_tensor(props):
        props = torch.cat(props) if props else None
    st = _Padded()
    st.B, st.dpi, st.cap, st.device, st.orig = B, dpi, cap, class_logits.device, orig
    if B == 0:
        return st
    dev = class_logits.device
    f32 = np.float32
    ratios = np.stack([orig[:, 1].astype(f32) / net[:, 1].astype(f32), orig[:, 0].astype(f32) / net[:, 0].astype(f32)], 1)   # width, height
    tables = _lib.host_to_device(np.concatenate([net.astype(f32).reshape(-1), ratios.astype(f32).reshape(-1)]), dev)
    offsets = _lib.ints_to_device(np.concatenate([[0], np.cumsum(counts)]), dev)
    arena = _arena(B, cap, dev)
    l = _lib.lib()
    _lib.check(l.cosy_det_decode(_lib.ptr(class_logits), _lib.ptr(box_regression), _lib.ptr(props), _lib.ptr(offsets), _lib.ptr(tables), R, C, B,
                                 float(score_thresh), cap, *map(_lib.ptr, arena), _lib.stream()))
    kept, n_kept = _arena_nms(arena, B, cap, nms_thresh, dpi)
    st.boxes_net = torch.empty((B * dpi, 4), dtype=torch.float32, device=dev)
    st.boxes_frame = torch.empty((B * dpi, 4), dtype=torch.float32, device=dev)
    st.src = torch.empty(B * dpi, dtype=torch.int32, device=dev)
    st.packed = torch.empty(2 * B + 2 * B * dpi, dtype=torch.int32, device=dev)
    _lib.check(l.cosy_det_gather(_lib.ptr(kept), _lib.ptr(n_kept), _lib.ptr(arena.counts), *map(_lib.ptr, arena[:4]), _lib.ptr(tables[2 * B:]), B, cap,
                                 dpi, _lib.ptr(st.boxes_net), _lib.ptr(st.boxes_frame), _lib.ptr(st.src), _lib.ptr(st.packed), _lib.stream()))
    return st


def _read(st):
    """THE device-to-host copy -> rows (indices of the padded rows that hold a detection, image by image, best score first), their
    image, category id and score"""
    B, dpi = st.B, st.dpi
    if B == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    host = st.packed.cpu().numpy()
    n_cand, n_kept = host[:B], host[B:2 * B]
    if (n_cand > st.cap).any():
        b = int(np.argmax(n_cand))
        raise ValueError(f'image {b} has {int(n_cand[b])} candidates above the score threshold, more than max_candidates = {st.cap}: raise '
                         f'max_candidates (at most {MAX_CANDIDATES}) or score_thresh; nothing is truncated silently')
    rows = np.concatenate([b * dpi + np.arange(int(n_kept[b])) for b in range(B)]).astype(np.int64)
    labels = host[2 * B:2 * B + B * dpi][rows].astype(np.int64)
    scores = host[2 * B + B * dpi:].view(np.float32)[rows]
    return rows, rows // dpi, labels, scores


def _select(t, rows, device):
    return t.index_select(0, torch.as_tensor(rows, dtype=torch.int64).to(device)) if len(rows) else t[:0]


def postprocess_detections(class_logits, box_regression, proposals, net_sizes, original_sizes=None, score_thresh=0.05, nms_thresh=0.5,
                           detections_per_img=100, counts=None, max_candidates=DEFAULT_CANDIDATES, return_source=False):
    """RoIHeads.postprocess_detections followed by the transform's postprocess, for all images of a batch at once.
    class_logits (R,C), box_regression (R,4C) float32 for the R proposals of all images; proposals: a list of (R_i,4) xyxy tensors, or
    one (R,4) tensor with counts = [R_i]; net_sizes: (height, width) of every image as the network saw it; original_sizes: of the
    frames (None: boxes stay at the network's scale).
    -> boxes (D,4) float32, scores (D) float32, labels (D) int64 category ids (1 .. C-1), batch_im_id (D) int64 on the device, by image,
    then by descending score[, with return_source also every detection's candidate index proposal-in-image * (C-1) + label - 1, int64]."""
    st = _run(class_logits, box_regression, proposals, net_sizes, original_sizes, counts, score_thresh, nms_thresh, detections_per_img,
              max_candidates)
    rows, im_ids, labels, scores = _read(st)
    dev = st.device
    if st.B == 0 or len(rows) == 0:
        out = (torch.empty((0, 4), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
               torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
        return out + (torch.empty(0, dtype=torch.int64, device=dev),) if return_source else out
    idx = torch.as_tensor(rows).to(dev)
    n = st.B * st.dpi
    out = (st.boxes_frame.index_select(0, idx), st.packed[2 * st.B + n:].view(torch.float32).index_select(0, idx),
           st.packed[2 * st.B:2 * st.B + n].index_select(0, idx).long(), idx // st.dpi)
    return out + (st.src.index_select(0, idx).long(),) if return_source else out


def paste_masks(mask_logits, boxes, labels, frame_size, mask_th=0.8, out=None):
    """maskrcnn_inference + paste_masks_in_image (padding 1) + the threshold: mask_logits (D,C,M,M) float32, boxes (D,4) xyxy float32 in
    the frame, labels (D) int = the channel of every detection (the category id), frame_size (H, W) -> (D,H,W) bool, every pixel
    written by one launch; the float (D,1,H,W) probabilities are never materialised.  A pixel outside the box holds the value 0 and is
    `0 > mask_th` like any other: false for mask_th >= 0, true for a negative one; a NaN mask_th gives all-false masks.  A label outside
    [0, C) pastes nothing: its whole plane holds 0 (an empty mask for mask_th >= 0)."""
    if not torch.is_tensor(mask_logits) or mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
        raise ValueError(f'mask_logits must be (D,C,M,M), got {tuple(mask_logits.shape) if torch.is_tensor(mask_logits) else type(mask_logits).__name__}')
    D, C, M = int(mask_logits.shape[0]), int(mask_logits.shape[1]), int(mask_logits.shape[2])
    if C < 1 or M < 1 or M > MAX_MASK_SIDE:
        raise ValueError(f'mask_logits must have C >= 1 channels of side 1 <= M <= {MAX_MASK_SIDE}, got C = {C}, M = {M}')
    mask_logits = _tensor(mask_logits, 'mask_logits', (D, C, M, M))
    boxes = _tensor(boxes, 'boxes', (D, 4))
    labels = _int_tensor(labels, 'labels', D)
    H, W = (int(v) for v in frame_size)
    if H < 1 or W < 1 or H * W >= 1 << 30:
        raise ValueError(f'frame_size must be a positive (H, W) below 2^30 pixels, got {(H, W)}')
    if out is None:
        _on_device(mask_logits=mask_logits, boxes=boxes, labels=labels)
        out = torch.empty((D, H, W), dtype=torch.bool, device=boxes.device)
    elif not torch.is_tensor(out) or out.dtype != torch.bool or tuple(out.shape) != (D, H, W) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous ({D},{H},{W}) bool tensor on the device')
    _on_device(mask_logits=mask_logits, boxes=boxes, labels=labels)
    _lib.check(_lib.lib().cosy_paste_masks(_lib.ptr(mask_logits), _lib.ptr(boxes), _lib.ptr(labels), D, C, M, H, W, float(mask_th),
                                           _lib.ptr(out.view(torch.uint8)), _lib.stream()))
    return out


def _filter(labels, scores, detection_th, one_instance_per_class):
    """Detector.get_detections' filters as io_formats.make_detections applies them -> positions kept, in output order"""
    keep = np.arange(len(scores))
    scores = scores.astype(np.float64)
    if detection_th is not None:
        keep = keep[scores[keep] > detection_th]
    if one_instance_per_class:
        ranked = keep[np.argsort(-scores[keep], kind='stable')]
        _, first = np.unique(labels[ranked].astype(str), return_index=True)
        keep = ranked[np.sort(first)]
    return keep


def detections_from_heads(class_logits, box_regression, proposals, net_sizes, original_sizes, category_id_to_label, mask_logits=None,
                          mask_head=None, detection_th=None, one_instance_per_class=False, output_masks=False, mask_th=0.8,
                          score_thresh=0.05, nms_thresh=0.5, detections_per_img=100, counts=None, max_candidates=DEFAULT_CANDIDATES):
    """Detector.get_detections from the heads' outputs on: the PandasTensorCollection with infos [batch_im_id, label, score], `bboxes`
    (D,4) float32 in the frame and, with output_masks, bool `masks` (D,H,W) (all frames of one size, original_sizes).
    category_id_to_label: mapping category id (1 .. C-1) -> label.  `detection_th` (strict >) and `one_instance_per_class` (the best
    score of every label over the whole batch, by descending score) apply BEFORE any mask exists.  Masks come from
      mask_head(boxes_net, batch_im_id) -> (D,C,M,M): called ONCE, with the surviving detections' boxes at the network's scale (D,4)
        and their images (D int64) -- the mask head never runs on a detection the filters dropped; or
      mask_logits (D0,C,M,M): computed earlier for the D0 rows postprocess_detections returns for the same arguments.
    One device-to-host copy (counts, labels, scores).  Nothing found: the empty collection make_detections returns."""
    st = _run(class_logits, box_regression, proposals, net_sizes, original_sizes, counts, score_thresh, nms_thresh, detections_per_img,
              max_candidates)
    if output_masks:
        if (mask_logits is None) == (mask_head is None):
            raise ValueError('output_masks needs exactly one of mask_logits and mask_head')
        if st.B and (st.orig != st.orig[0]).any():
            raise ValueError(f'output_masks needs all frames of one size, got {st.orig.tolist()}')
    rows, im_ids, cat_ids, scores = _read(st)
    dev = st.device
    if len(rows) == 0:
        return empty_detections(dev)
    labels = np.array([str(category_id_to_label[int(c)]) for c in cat_ids], dtype=object)
    keep = _filter(labels, scores, detection_th, one_instance_per_class)
    infos = pd.DataFrame({'batch_im_id': im_ids[keep], 'label': labels[keep], 'score': scores[keep].astype(np.float64)})
    idx = torch.as_tensor(rows[keep], dtype=torch.int64).to(dev)
    fields = {'bboxes': st.boxes_frame.index_select(0, idx)}
    if output_masks:
        D = len(keep)
        if mask_head is not None:
            logits = mask_head(st.boxes_net.index_select(0, idx), idx // st.dpi)
        else:
            if not torch.is_tensor(mask_logits) or mask_logits.dim() != 4 or mask_logits.shape[0] != len(rows) or not mask_logits.is_cuda:
                raise ValueError(f'mask_logits must hold one (C,M,M) row on the device for each of the {len(rows)} detections of postprocess_detections')
            logits = mask_logits.index_select(0, torch.as_tensor(keep, dtype=torch.int64).to(dev))
        if not torch.is_tensor(logits) or logits.dim() != 4 or logits.shape[0] != D:
            raise ValueError(f'the mask head must return (D,C,M,M) logits for the {D} boxes it was given')
        fields['masks'] = paste_masks(logits, fields['bboxes'], torch.as_tensor(cat_ids[keep], dtype=torch.int32).to(dev),
                                      (int(st.orig[0, 0]), int(st.orig[0, 1])), mask_th)
    return tc.PandasTensorCollection(infos=infos, **fields)

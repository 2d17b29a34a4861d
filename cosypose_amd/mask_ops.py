"""Annotations read off instance-id masks on the device: pixel counts and boxes per id, the visible ids, per-object binary masks and the
detection targets.  What the reference does on the CPU, one frame and one id at a time (cosypose/datasets/utils.py:27-40
make_detections_from_segmentation, datasets/wrappers/visibility_wrapper.py, the visibility filter of datasets/pose_dataset.py:90-105
and datasets/detection_dataset.py:61-80), runs here as one launch sequence per batch (HIP: csrc/kernels_det.hip) on masks that stay
where HipSceneRenderer and augment_batch leave them.

masks: (B,H,W) -- or (H,W), read as one image -- of uint8, bool (read as uint8) or int32, on the device.  A box holds inclusive pixel
indices x1, y1, x2, y2 (np.min / np.max of np.where); pixels whose value lies outside [0, n_ids) are skipped, which covers the scene
renderer's -1 background.  Integer arithmetic only: results are exact and the same from run to run.
"""
import numpy as np
import torch

from . import _lib

MAX_IDS = 1024


def _masks(masks):
    _lib.require_device(masks)
    if masks.dim() == 2:
        masks = masks.unsqueeze(0)
    if masks.dim() != 3:
        raise ValueError(f'masks must be (B,H,W) or (H,W), got {tuple(masks.shape)}')
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    if masks.dtype == torch.uint8:
        dtype = _lib.COSY_MASK_U8
    elif masks.dtype == torch.int32:
        dtype = _lib.COSY_MASK_I32
    else:
        raise TypeError(f'masks must be uint8, bool or int32, got {masks.dtype}')
    return masks.contiguous(), dtype


def mask_instance_stats(masks, n_ids=None):
    """-> (B, n_ids, 5) int32 on the device: count, x1, y1, x2, y2 of every id in [0, n_ids); an absent id gives 0, -1, -1, -1, -1.
    n_ids defaults to 256 for uint8 / bool masks and must be given for int32 ones (at most 1024)."""
    masks, dtype = _masks(masks)
    if n_ids is None:
        if dtype != _lib.COSY_MASK_U8:
            raise ValueError('n_ids must be given for int32 masks')
        n_ids = 256
    B, H, W = masks.shape
    stats = torch.empty((B, int(n_ids), 5), dtype=torch.int32, device=masks.device)
    _lib.check(_lib.lib().cosy_mask_instance_stats(_lib.ptr(masks), dtype, B, H, W, int(n_ids), _lib.ptr(stats), _lib.stream()))
    return stats


def make_detections_from_segmentation(masks, n_ids=None):
    """The reference's function of the same name: one dict {id: tensor([x1, y1, x2, y2])} per mask, present ids only, ascending (int64
    tensors on the masks' device, as the reference's).  One stats call and one device-to-host copy serve the whole batch.  (B,1,H,W)
    masks with B = 1 are accepted as the reference accepts them."""
    if masks.dim() == 4:
        assert masks.shape[0] == 1
        masks = masks.squeeze(0)
    stats = mask_instance_stats(masks, n_ids)
    host = stats.cpu().numpy()
    detections = []
    for stats_n in host:
        present = np.flatnonzero(stats_n[:, 0] > 0)
        boxes = torch.from_numpy(stats_n[present, 1:].astype(np.int64)).to(stats.device)
        detections.append({int(i): box for i, box in zip(present, boxes)})
    return detections


def visible_ids(masks, n_ids=None):
    """VisibilityWrapper's rule: per mask, the ids greater than 0 that own at least one pixel -> list of int64 numpy arrays, ascending"""
    host = mask_instance_stats(masks, n_ids)[:, :, 0].cpu().numpy()
    return [np.flatnonzero(c[1:] > 0).astype(np.int64) + 1 for c in host]


def instance_masks(masks, row_image, row_id):
    """-> (N,H,W) uint8 on the device, out[n] = masks[row_image[n]] == row_id[n].  row_image / row_id: N ints each (lists, numpy or
    tensors).  A row whose image index lies outside [0, B) gives zeros."""
    masks, dtype = _masks(masks)
    B, H, W = masks.shape
    row_image = _lib.ints_to_device(row_image, masks.device).reshape(-1)
    row_id = _lib.ints_to_device(row_id, masks.device).reshape(-1)
    if row_image.shape != row_id.shape:
        raise ValueError(f'row_image and row_id differ in length: {row_image.numel()} and {row_id.numel()}')
    N = row_image.numel()
    out = torch.empty((N, H, W), dtype=torch.uint8, device=masks.device)
    _lib.check(_lib.lib().cosy_instance_masks(_lib.ptr(masks), dtype, _lib.ptr(row_image), _lib.ptr(row_id), B, H, W, N, _lib.ptr(out),
                                              _lib.stream()))
    return out


def detection_targets(masks, image_ids, ids_in_segm, min_area=50, n_ids=None):
    """DetectionDataset's targets (detection_dataset.py:61-74) for N objects of a batch: object n is id ids_in_segm[n] of image
    image_ids[n].  -> dict of device tensors: boxes (n_keep,4) float32, the inclusive box of the object's pixels; area (n_keep) float32
    = (x2 - x1) * (y2 - y1) of that box; masks (n_keep,H,W) uint8; keep (N) bool = area > min_area (strictly, as the reference has
    it).  An object without a pixel (or whose ids lie outside the tables) has area 0."""
    stats = mask_instance_stats(masks, n_ids)
    B, n_ids = stats.shape[:2]
    image_ids = _lib.ints_to_device(image_ids, stats.device).reshape(-1).long()
    ids_in_segm = _lib.ints_to_device(ids_in_segm, stats.device).reshape(-1).long()
    inside = (image_ids >= 0) & (image_ids < B) & (ids_in_segm >= 0) & (ids_in_segm < n_ids)
    rows = stats[image_ids.clamp(0, B - 1), ids_in_segm.clamp(0, n_ids - 1)] if B else stats.new_zeros((len(image_ids), 5))
    boxes = torch.where(inside[:, None], rows[:, 1:], torch.full_like(rows[:, 1:], -1)).float()
    area = (boxes[:, 3] - boxes[:, 1]) * (boxes[:, 2] - boxes[:, 0])
    keep = area > min_area
    kept = torch.nonzero(keep).reshape(-1)
    return dict(boxes=boxes[kept], area=area[kept], masks=instance_masks(masks, image_ids[kept], ids_in_segm[kept]), keep=keep)

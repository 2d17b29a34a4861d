"""Frames to the training size on the device: the step every frame of the reference's PoseDataset and DetectionDataset goes through first,
CropResizeToAspectAugmentation(resize=(640, 480)) (cosypose/datasets/augmentations.py:137-192, called at pose_dataset.py:80 and
detection_dataset.py:50), for frames of the target aspect.  DESIGN.md section 18 holds the definition; csrc/kernels_frames.hip the kernel.

    out = resize_frames(raw_images, resize=(640, 480), masks=raw_masks, K=K, boxes=True)
    images = augment_batch(out.images, recs, masks=out.masks, backgrounds=backgrounds)

The image goes through float32 bilinear interpolation with half-pixel centres and a truncating cast to bytes, the instance mask through
nearest, K through get_K_crop_resize; the boxes are read again off the resized masks (mask_ops.mask_instance_stats).  Everything that
divides -- the taps and weights of an axis, the nearest indices, u / 255, K -- is computed here in numpy float32, one rounding per
operation, and kept per (n_in, n_out); a call uploads one buffer -- the per-frame descriptors and the tables of the axes it uses --
and makes ONE launch for images and masks, whatever the mix of sizes.  A frame whose aspect is not the target's is refused: the reference
crops it with torchvision's roi_pool, which is not restated here.  There is no CPU path: tensors on the CPU are refused.
"""
import collections
import functools

import numpy as np

from . import _lib
from ._tables import TablePacker

F32 = np.float32
# cosy_frame_item_t
ITEM_DTYPE = np.dtype([('image', '<u8'), ('mask', '<u8'), ('h', '<i4'), ('w', '<i4'), ('xb', '<i4'), ('yb', '<i4'), ('xn', '<i4'), ('yn', '<i4')])
assert ITEM_DTYPE.itemsize == 40

ResizedFrames = collections.namedtuple('ResizedFrames', 'images masks K crop_resize_bbox stats')
ResizedFrames.__doc__ = """images (N,3,H,W) uint8; masks (N,H,W) uint8 or None; K (N,3,3) float32 (on the side it came from) or None;
crop_resize_bbox (N,4) float64 numpy, the reference's orig_camera['crop_resize_bbox']; stats (N,n_ids,5) int32 = mask_instance_stats of
`masks` when boxes were asked for, else None"""


@functools.lru_cache(maxsize=1)
def byte_values():
    """float32(u) / 255f for u in 0..255, as int32 bit patterns"""
    p = (np.arange(256, dtype=F32) / F32(255)).astype(F32).view(np.int32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=256)
def axis_tables(n_in, n_out):
    """-> (taps (n_out,4) int32 = i0, i1, bits of l0, bits of l1; nearest (n_out,) int32) of one axis, numpy float32 with one rounding
    per operation; read-only, cached"""
    scale = F32(n_in) / F32(n_out)
    i = np.arange(n_out, dtype=F32)
    real = np.maximum(scale * (i + F32(0.5)) - F32(0.5), F32(0))
    i0 = real.astype(np.int32)
    i1 = np.minimum(i0 + 1, n_in - 1).astype(np.int32)
    l1 = np.clip(real - i0.astype(F32), F32(0), F32(1)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    taps = np.stack([i0, i1, l0.view(np.int32), l1.view(np.int32)], axis=1).astype(np.int32)
    nearest = np.minimum(np.floor(i * scale).astype(np.int32), n_in - 1).astype(np.int32)
    taps.setflags(write=False)
    nearest.setflags(write=False)
    return taps, nearest


def axis_offsets(packer, n_in, n_out):
    """-> offsets of (tap table, nearest table) of an axis in a _tables.TablePacker, placed on first use, the taps' a multiple of 4 ints"""
    key = (n_in, n_out)
    return packer.offsets.get(key) or packer.place(key, *axis_tables(n_in, n_out), align_ints=4)


def resized_K(K, h, w, H, W):
    """get_K_crop_resize(K, boxes=(0, 0, w, h), orig_size=(h, w), crop_resize=(H, W)) of the reference (lib3d/camera_geometry.py:45-87)
    for one (3,3) K, in float32 and in its order of operations"""
    K = np.asarray(K, F32)
    new_K = K.copy()
    x1, y1, x2, y2 = F32(0), F32(0), F32(w), F32(h)
    final_width, final_height = F32(max(H, W)), F32(min(H, W))
    crop_width, crop_height = x2 - x1, y2 - y1
    crop_cj, crop_ci = (x1 + x2) / F32(2), (y1 + y2) / F32(2)
    cx = K[0, 2] + (crop_width - F32(1)) / F32(2) - crop_cj
    cy = K[1, 2] + (crop_height - F32(1)) / F32(2) - crop_ci
    center_x, center_y = (crop_width - F32(1)) / F32(2), (crop_height - F32(1)) / F32(2)
    scale_x, scale_y = final_width / crop_width, final_height / crop_height
    new_K[0, 0] = scale_x * K[0, 0]
    new_K[1, 1] = scale_y * K[1, 1]
    new_K[0, 2] = (final_width - F32(1)) / F32(2) + scale_x * (cx - center_x)
    new_K[1, 2] = (final_height - F32(1)) / F32(2) + scale_y * (cy - center_y)
    return new_K


def _check_resize(resize):
    try:
        a, b = (int(v) for v in resize)
    except (TypeError, ValueError):
        raise ValueError(f'resize must be two positive integers, got {resize!r}') from None
    if a < 1 or b < 1 or (a, b) != tuple(resize):
        raise ValueError(f'resize must be two positive integers, got {resize!r}')
    return min(a, b), max(a, b)


def check_aspect(i, h, w, H, W):
    """the reference's test (augmentations.py:157) for frame i of h x w against the target H x W"""
    if not np.isclose(w / h, W / H):
        raise ValueError(f'frame {i} is {h}x{w}: its aspect w/h = {w / h:.6g} is not the target\'s {W / H:.6g} ({H}x{W}); the '
                         'reference crops such a frame with roi_pool, which is not served')


def _planes(what, value, dim, torch):
    """a (N,...) tensor or a list of tensors -> list of contiguous uint8 tensors of `dim` dimensions"""
    if isinstance(value, torch.Tensor):
        _lib.require_device(value)
        if value.dtype != torch.uint8 or value.dim() != dim + 1:
            raise ValueError(f'{what} must be a uint8 tensor of {dim + 1} dimensions or a list of uint8 tensors of {dim}, got {tuple(value.shape)} {value.dtype}')
        return list(value.contiguous().unbind(0))
    planes = list(value)
    for t in planes:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'a list of {what} holds uint8 tensors, got {type(t)!r}')
    _lib.require_device(*planes)
    for t in planes:
        if t.dtype != torch.uint8 or t.dim() != dim:
            raise ValueError(f'a list of {what} holds uint8 tensors of {dim} dimensions, got {tuple(t.shape)} {t.dtype}')
    return [t.contiguous() for t in planes]


def resize_frames(images, resize=(640, 480), masks=None, K=None, boxes=False, out=None, out_masks=None):
    """images: a list of (3,h_i,w_i) uint8 device tensors whose sizes may differ, or one (N,3,h,w) tensor.  masks: a list of (h_i,w_i)
    uint8 device tensors or one (N,h,w), or None.  K: (N,3,3), tensor on either side or numpy, or None.  (H, W) = (min(resize),
    max(resize)), as the reference has it.  boxes=True (needs masks) also returns mask_instance_stats of the resized masks; the rows of
    frames that were already at (H, W) are there too, but the reference leaves the boxes of such a frame as they were, and so should the
    caller.  out / out_masks: contiguous uint8 tensors of the results' shapes to write into.  -> ResizedFrames.
    A frame whose w / h is not np.isclose to W / H raises ValueError before anything is launched."""
    import torch
    H, W = _check_resize(resize)
    frames = _planes('images', images, 3, torch)
    n = len(frames)
    if n == 0:
        raise ValueError('resize_frames needs at least one frame')
    device = frames[0].device
    if any(t.shape[0] != 3 for t in frames) or any(t.device != device for t in frames):
        raise ValueError('the images have 3 channels and live on one device')
    if any(t.shape[1] < 1 or t.shape[2] < 1 for t in frames):
        raise ValueError('a frame without pixels cannot be resized')
    sizes = [(int(t.shape[1]), int(t.shape[2])) for t in frames]
    for i, (h, w) in enumerate(sizes):
        check_aspect(i, h, w, H, W)
    mask_planes = None
    if masks is not None:
        mask_planes = _planes('masks', masks, 2, torch)
        if len(mask_planes) != n or any(tuple(m.shape) != s for m, s in zip(mask_planes, sizes)) or any(m.device != device for m in mask_planes):
            raise ValueError('masks holds one (h_i,w_i) mask per frame, of its frame\'s size and on its device')
    elif boxes or out_masks is not None:
        raise ValueError('boxes=True and out_masks= need masks')
    K_host = None
    if K is not None:
        K_host = (K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).astype(F32)
        if K_host.shape != (n, 3, 3):
            raise ValueError(f'K must be ({n},3,3), got {K_host.shape}')
    out = _lib.out_or_new(out, 'out', (n, 3, H, W), torch.uint8, device)
    if mask_planes is not None:
        out_masks = _lib.out_or_new(out_masks, 'out_masks', (n, H, W), torch.uint8, device)

    # one table: the 256 byte values, then the tap and nearest tables of every axis this call uses; one descriptor per frame with their offsets
    packer = TablePacker(byte_values())
    items = np.zeros(n, ITEM_DTYPE)
    items['image'] = [t.data_ptr() for t in frames]
    if mask_planes is not None:
        items['mask'] = [m.data_ptr() for m in mask_planes]
    items['h'], items['w'] = zip(*sizes)
    resized = [s != (H, W) for s in sizes]
    at = {(h, w): axis_offsets(packer, w, W) + axis_offsets(packer, h, H) for h, w in dict.fromkeys(sizes) if (h, w) != (H, W)}
    items['xb'], items['xn'], items['yb'], items['yn'] = zip(*(at.get(s, (0, 0, 0, 0)) for s in sizes))
    blob_d, items_p, tables_p, n_tables = packer.upload(items, device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().cosy_resize_frames_u8(items_p, n, H, W, tables_p, n_tables, 0, _lib.ptr(out), _lib.ptr(out_masks), _lib.stream()))
        stats = None
        if boxes:
            from .mask_ops import mask_instance_stats
            stats = mask_instance_stats(out_masks)

    bbox = np.array([(0.0, 0.0, w, h) if r else (0.0, 0.0, w - 1, h - 1) for (h, w), r in zip(sizes, resized)], np.float64).reshape(n, 4)
    K_out = None
    if K_host is not None:
        K_new = np.stack([resized_K(k, h, w, H, W) if r else k for k, (h, w), r in zip(K_host, sizes, resized)])
        K_out = torch.from_numpy(K_new)
        if isinstance(K, torch.Tensor) and K.is_cuda:
            K_out = _lib.host_to_device(K_out, K.device)
    return ResizedFrames(out, out_masks, K_out, bbox, stats)

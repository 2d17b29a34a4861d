"""Training augmentations of the reference's PoseDataset.get_data (cosypose/datasets/pose_dataset.py:82-87, datasets/augmentations.py)
on the device, on the collated uint8 batch: background paste, Pillow's GaussianBlur and ImageEnhance Sharpness / Contrast / Brightness /
Color, the float32 grey conversion.  The bytes are Pillow 12's (csrc/kernels_aug.hip).

The random draws stay on the host and in the reference's order, one sample at a time, so that a dataset can interleave its own draws (the
`random.sample` of the object that follows in get_data) and a seeded run reproduces the reference's sequence:

    recs = [draw_sample_params(random, gray_augmentation=True, n_backgrounds=len(backgrounds)) for _ in range(B)]
    images = augment_batch(images_u8, recs, masks=masks_u8, backgrounds=backgrounds_u8)       # (B,3,H,W) uint8, as h_pose takes it

There is no CPU path: tensors on the CPU are refused.
"""
import random

import numpy as np

from . import _lib

GATE, SHARPNESS, CONTRAST, BRIGHTNESS, COLOR, GRAY = (_lib.AUG_GATE, _lib.AUG_SHARPNESS, _lib.AUG_CONTRAST, _lib.AUG_BRIGHTNESS, _lib.AUG_COLOR,
                                                       _lib.AUG_GRAY)
RGB_GATE_P = 0.8
# stage -> (p, factor interval, present bit), in the order PoseDataset applies them (pose_dataset.py:54-60)
STAGES = (('sharpness', 0.3, (0., 50.), SHARPNESS), ('contrast', 0.3, (0.2, 50.), CONTRAST),
          ('brightness', 0.5, (0.1, 6.0), BRIGHTNESS), ('color', 0.3, (0., 20.), COLOR))
BLUR_INTERVAL = (1, 3)
GRAY_P = 0.5
# cosy_aug_params_t
PARAMS_DTYPE = np.dtype([('bg', '<i4'), ('flags', '<i4'), ('k', '<i4'), ('sharpness', '<f4'), ('contrast', '<f4'), ('brightness', '<f4'),
                         ('color', '<f4'), ('reserved', '<i4')])
assert PARAMS_DTYPE.itemsize == 32


def draw_sample_params(rng=random, rgb_augmentation=True, gray_augmentation=False, background_p=0.3, n_backgrounds=0):
    """The draws get_data makes for ONE sample between the resize and the object selection, in its order, from `rng` (the `random`
    module or a random.Random): BackgroundAugmentation.__call__ when n_backgrounds > 0, the 0.8 gate (strict <), PillowBlur (its p is
    never read: always k = randint(1, 3)), Sharpness / Contrast / Brightness / Color (random() <= p, then uniform), GrayScale with
    gray_augmentation.  Returns the record: dict(bg = background row or -1, gate, k, sharpness / contrast / brightness / color = factor
    or None, gray)."""
    rec = dict(bg=-1, gate=False, k=0, sharpness=None, contrast=None, brightness=None, color=None, gray=False)
    if n_backgrounds > 0 and rng.random() <= background_p:
        rec['bg'] = rng.randint(0, n_backgrounds - 1)
    if rgb_augmentation and rng.random() < RGB_GATE_P:
        rec['gate'] = True
        rec['k'] = rng.randint(*BLUR_INTERVAL)
        for name, p, interval, _ in STAGES:
            if rng.random() <= p:
                rec[name] = rng.uniform(*interval)
        if gray_augmentation and rng.random() <= GRAY_P:
            rec['gray'] = True
    return rec


def pack_params(records):
    """list of records -> (B,) numpy array of PARAMS_DTYPE, the host image of the device table (factors become float32, as Pillow's
    ImagingBlend takes them)."""
    table = np.zeros(len(records), PARAMS_DTYPE)
    for row, rec in zip(table, records):
        row['bg'] = rec['bg']
        if rec['bg'] < -1:
            raise ValueError(f"background row {rec['bg']}")
        if not rec['gate']:
            continue
        if rec['k'] not in (1, 2, 3):
            raise ValueError(f"blur radius {rec['k']!r}: GaussianBlur(k) is served for k in 1, 2, 3")
        flags = GATE | (GRAY if rec['gray'] else 0)
        for name, _, _, bit in STAGES:
            if rec[name] is not None:
                flags |= bit
                row[name] = rec[name]
        row['flags'], row['k'] = flags, rec['k']
    return table


def unpack_params(table):
    """the inverse of pack_params (factors come back as the float32 values the device sees)"""
    out = []
    for row in np.asarray(table):
        flags = int(row['flags'])
        rec = dict(bg=int(row['bg']), gate=bool(flags & GATE), k=int(row['k']) if flags & GATE else 0, gray=bool(flags & GRAY))
        for name, _, _, bit in STAGES:
            rec[name] = float(row[name]) if flags & bit else None
        out.append(rec)
    return out


def params_to_device(params, device):
    """records / packed table -> (B,8) int32 device tensor (through pinned memory: the stream is not drained)"""
    import torch
    if isinstance(params, torch.Tensor):
        if params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != 8:
            raise ValueError('a parameter table is (B,8) int32, the bytes of pack_params')
        return params.to(device).contiguous()
    table = params if isinstance(params, np.ndarray) and params.dtype == PARAMS_DTYPE else pack_params(list(params))
    return _lib.host_to_device(np.ascontiguousarray(table).view(np.int32).reshape(len(table), 8), device)


def augment_batch(images, params, masks=None, backgrounds=None, out=None):
    """images (B,3,H,W) uint8 on the device; params: a list of draw_sample_params records, pack_params's table, or that table on the
    device as (B,8) int32; masks (B,H,W) uint8 and backgrounds (N,3,H,W) uint8, already at frame size, are needed only where a record
    names a background.  Returns `out` (default: a new tensor) with the same shape and dtype; out may be `images` itself."""
    import torch
    _lib.require_device(images, masks, backgrounds, out)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f'images must be (B,3,H,W) uint8, got {tuple(images.shape)} {images.dtype}')
    B, _, H, W = images.shape
    images = images.contiguous()
    n_bg = 0
    if masks is not None and backgrounds is not None:
        if masks.dtype != torch.uint8 or tuple(masks.shape) != (B, H, W):
            raise ValueError(f'masks must be ({B},{H},{W}) uint8, got {tuple(masks.shape)} {masks.dtype}')
        if backgrounds.dtype != torch.uint8 or backgrounds.dim() != 4 or tuple(backgrounds.shape[1:]) != (3, H, W):
            raise ValueError(f'backgrounds must be (N,3,{H},{W}) uint8, got {tuple(backgrounds.shape)} {backgrounds.dtype}')
        masks, backgrounds, n_bg = masks.contiguous(), backgrounds.contiguous(), backgrounds.shape[0]
    elif (masks is None) != (backgrounds is None):
        raise ValueError('masks and backgrounds go together')
    if not isinstance(params, torch.Tensor):
        table = params if isinstance(params, np.ndarray) and params.dtype == PARAMS_DTYPE else pack_params(list(params))
        if len(table) and int(table['bg'].max()) >= n_bg:
            raise ValueError(f"a record names background {int(table['bg'].max())} and {n_bg} are given")
        params = table
    table_d = params_to_device(params, images.device)
    if table_d.shape[0] != B:
        raise ValueError(f'{table_d.shape[0]} parameter records for {B} images')
    if out is None:
        out = torch.empty_like(images)
    elif out.dtype != torch.uint8 or out.shape != images.shape or not out.is_contiguous() or out.device != images.device:
        raise ValueError('out must be a contiguous uint8 tensor of the shape and device of images')
    if B == 0:
        return out
    lib = _lib.lib()
    ws_bytes = lib.cosy_augment_workspace_bytes(B, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=images.device)
    _lib.check(lib.cosy_augment_batch(_lib.ptr(images), _lib.ptr(masks) if n_bg else None, _lib.ptr(backgrounds) if n_bg else None, n_bg,
                                      _lib.ptr(table_d), B, H, W, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream()))
    return out

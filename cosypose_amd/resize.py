"""Pillow's Image.resize of 8-bit images on the device, byte for byte: the step of the reference's BackgroundAugmentation.__call__
(cosypose/datasets/augmentations.py:120-124) that brings a background of any size to the frame before the paste.  The bytes are
Pillow 12's (csrc/kernels_resize.hip):

    backgrounds = resize_images(raw_list, (H, W))                     # list of (3,h_i,w_i) uint8 device tensors -> (N,3,H,W) uint8
    images = augment_batch(images_u8, recs, masks=masks_u8, backgrounds=backgrounds)

'bicubic' is what im.resize(size) does without a filter argument for RGB and L images, 'bilinear' is Image.BILINEAR.  The coefficient
tables of an axis are computed once on the host, in double, by the library's cosy_resize_coeffs and kept per (in, out, filter); a call
uploads one buffer -- the per-image descriptors and the tables of the axes it uses -- and makes ONE call of the library, whatever the
mix of sizes.  There is no CPU path: tensors on the CPU are refused.
"""
import ctypes
import functools

import numpy as np

from . import _lib
from ._tables import TablePacker

FILTERS = {'bilinear': _lib.RESIZE_BILINEAR, 'bicubic': _lib.RESIZE_BICUBIC}
# cosy_resize_item_t
ITEM_DTYPE = np.dtype([('src', '<u8'), ('h', '<i4'), ('w', '<i4'), ('hb', '<i4'), ('hk', '<i4'), ('hks', '<i4'), ('vb', '<i4'), ('vk', '<i4'),
                       ('vks', '<i4')])
assert ITEM_DTYPE.itemsize == 40


@functools.lru_cache(maxsize=256)
def axis_tables(n_in, n_out, resample):
    """-> (bounds (n_out,2) int32 = first tap and number of taps, k (n_out,ksize) int32 coefficients in 2^-22) of one axis, from the
    library's host routine (no device is touched); read-only, cached"""
    lib = _lib.lib()
    filt = FILTERS[resample]
    ksize = lib.cosy_resize_ksize(n_in, n_out, filt)
    _lib.check(min(ksize, 0))
    bounds, k = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    _lib.check(min(lib.cosy_resize_coeffs(n_in, n_out, filt, bounds.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), k.size), 0))
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def _check_size(size):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f'size must be (H, W), got {size!r}') from None
    if H < 1 or W < 1 or (H, W) != tuple(size):
        raise ValueError(f'size must be two positive integers (H, W), got {size!r}')
    return H, W


def resize_images(images, size, resample='bicubic', out=None):
    """images: a (N,C,h,w) uint8 device tensor, or a list of (C,h_i,w_i) uint8 device tensors whose sizes may differ; C is 1 or 3.
    size = (H, W).  resample: 'bicubic' (Pillow's default) or 'bilinear'.  Returns `out` (default: a new tensor), (N,C,H,W) uint8 on the
    device, a contiguous uint8 tensor of that shape when given.  An image already at (H, W) is copied."""
    import torch
    H, W = _check_size(size)
    if resample not in FILTERS:
        raise ValueError(f"resample must be 'bicubic' or 'bilinear', got {resample!r} (nearest, lanczos and hamming are not served)")
    if isinstance(images, torch.Tensor):
        _lib.require_device(images, out)
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise ValueError(f'images must be (N,C,h,w) uint8 or a list of (C,h,w) uint8, got {tuple(images.shape)} {images.dtype}')
        batch = images.contiguous()
        C = batch.shape[1]
        planes = list(batch.unbind(0)) if batch.shape[0] else []
        device = batch.device
        if batch.shape[0] == 0 and C in (1, 3):
            return _lib.out_or_new(out, 'out', (0, C, H, W), torch.uint8, device)
    else:
        planes = list(images)
        _lib.require_device(*planes, out)
        for t in planes:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
                raise ValueError('a list of images holds (C,h,w) uint8 tensors, got ' + (f'{tuple(t.shape)} {t.dtype}' if isinstance(t, torch.Tensor) else repr(type(t))))
        if not planes:
            if out is None:
                raise ValueError('an empty list of images names neither its channels nor its device: pass a (0,C,h,w) tensor, or out=')
            _lib.require_device(out)
            if out.dim() != 4 or out.shape[1] not in (1, 3):
                raise ValueError('out must be a contiguous uint8 tensor of the shape and device of the result')
            return _lib.out_or_new(out, 'out', (0, out.shape[1], H, W), torch.uint8, out.device)
        C, device = planes[0].shape[0], planes[0].device
        if any(t.shape[0] != C for t in planes) or any(t.device != device for t in planes):
            raise ValueError('the images of a list have the same number of channels and live on one device')
        planes = [t.contiguous() for t in planes]
    if C not in (1, 3):
        raise ValueError(f'images have 1 or 3 channels, got {C}')
    if any(t.shape[1] < 1 or t.shape[2] < 1 for t in planes):
        raise ValueError('an image without pixels cannot be resized')
    n = len(planes)
    out = _lib.out_or_new(out, 'out', (n, C, H, W), torch.uint8, device)

    # one table of all the axes this call uses, and one descriptor per image with its offsets into it (in ints)
    packer = TablePacker(what='coefficient tables')

    def axis(n_in, n_out):
        if n_in == n_out:
            return 0, 0, 0                                   # ksize 0: the pass is skipped
        bounds, k = axis_tables(n_in, n_out, resample)
        return (*packer.place((n_in, n_out), bounds, k), k.shape[1])

    items = np.zeros(n, ITEM_DTYPE)
    items['src'] = [t.data_ptr() for t in planes]
    heights, widths = [t.shape[1] for t in planes], [t.shape[2] for t in planes]
    rows, cols = {w: axis(w, W) for w in dict.fromkeys(widths)}, {h: axis(h, H) for h in dict.fromkeys(heights)}
    items['h'], items['w'] = heights, widths
    items['hb'], items['hk'], items['hks'] = zip(*(rows[w] for w in widths))
    items['vb'], items['vk'], items['vks'] = zip(*(cols[h] for h in heights))
    blob_d, items_p, tables_p, n_tables = packer.upload(items, device)
    max_h = max(t.shape[1] for t in planes)
    lib = _lib.lib()
    with torch.cuda.device(device):
        ws_bytes = lib.cosy_resize_workspace_bytes(n, C, max_h, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        _lib.check(lib.cosy_resize_u8(items_p, n, C, H, W, max_h, tables_p, n_tables, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream()))
    return out


"""numpy restatement of DESIGN.md section 18: the frames' own resize (the reference's CropResizeToAspectAugmentation, cosypose/datasets/
augmentations.py:137-192, for frames of the target aspect) -- the image through float32 bilinear interpolation with half-pixel centres,
the instance mask through nearest, K through get_K_crop_resize, the boxes off the resized mask.  Independent of the package: nothing
here imports cosypose_amd.  Also the float64-exact value of every output byte, which names the pixels where the reference's own bytes
depend on which of torch's kernels ran (`near_integer`), and the parity rule that both test files hold the fixture to.

A fused multiply-add fma(a, b, c) of float32 values is emulated as float32(float64(a) * float64(b) + float64(c)): the product is exact
in float64, the sum is rounded to 53 bits and then to 24.  That double rounding differs from the single one only when the float64 sum was
inexact AND lies within a few units of its last place of a midpoint between two float32 values; `fma32` raises DoubleRounding when it
meets such a sum rather than return a value that may be off by one unit.
"""
import numpy as np

F32 = np.float32
DELTA = 1e-4                                   # |exact - nearest integer| below which a byte counts as near-integer


class DoubleRounding(ArithmeticError):
    pass


def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, one rounding; raises DoubleRounding where the emulation cannot promise that"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    x = a * b                                  # exact: 24 + 24 bits
    s = x + c
    bb = s - x
    err = (x - (s - bb)) + (c - bb)            # TwoSum: the rounding error of the float64 sum, exactly
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    lo = np.where(r64 <= s, r, np.nextafter(r, F32(-np.inf)))
    hi = np.nextafter(lo, F32(np.inf))
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    risky = (err != 0) & (np.abs(s - mid) <= 2.0 ** -50 * np.abs(s))
    if risky.any():
        raise DoubleRounding(f'{int(risky.sum())} sums lie within 2^-50 of a float32 midpoint: the float64 emulation of fmaf is not safe there')
    return r


def out_size(resize):
    return int(min(resize)), int(max(resize))


def axis(n_in, n_out):
    """-> i0, i1 (int64), l0, l1 (float32) of every output index of one axis"""
    scale = F32(n_in) / F32(n_out)
    i = np.arange(n_out, dtype=F32)
    real = np.maximum(scale * (i + F32(0.5)) - F32(0.5), F32(0))
    assert real.dtype == F32
    i0 = real.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(real - i0.astype(F32), F32(0), F32(1)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def two_tap(p, H, W):
    """(C,h,w) float32 of looked-up values -> (C,H,W) float32: the three fused multiply-adds and three lone products of section 18"""
    y0, y1, ly0, ly1 = axis(p.shape[1], H)
    x0, x1, lx0, lx1 = axis(p.shape[2], W)
    lx0, lx1 = lx0[None, None, :], lx1[None, None, :]
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    p00, p01 = p[:, y0][:, :, x0], p[:, y0][:, :, x1]
    p10, p11 = p[:, y1][:, :, x0], p[:, y1][:, :, x1]
    top = fma32(lx0, p00, (lx1 * p01).astype(F32))
    bot = fma32(lx0, p10, (lx1 * p11).astype(F32))
    return fma32(ly0, top, (ly1 * bot).astype(F32))


def two_tap_float64(p, H, W):
    """the same bilinear form of (C,h,w) values with the float32 weights, every product and sum in float64"""
    p = p.astype(np.float64)
    y0, y1, ly0, ly1 = axis(p.shape[1], H)
    x0, x1, lx0, lx1 = axis(p.shape[2], W)
    lx0, lx1 = lx0.astype(np.float64)[None, None, :], lx1.astype(np.float64)[None, None, :]
    ly0, ly1 = ly0.astype(np.float64)[None, :, None], ly1.astype(np.float64)[None, :, None]
    top = lx0 * p[:, y0][:, :, x0] + lx1 * p[:, y0][:, :, x1]
    bot = lx0 * p[:, y1][:, :, x0] + lx1 * p[:, y1][:, :, x1]
    return ly0 * top + ly1 * bot


def image_float(image, H, W):
    """(C,h,w) uint8 -> (C,H,W) float32, the interpolated value in [0, 1] (what F.interpolate returns)"""
    return two_tap((np.arange(256, dtype=F32) / F32(255)).astype(F32)[image], H, W)


def to_bytes(v):
    return np.trunc((v * F32(255)).astype(F32)).astype(np.uint8)


def image_bytes(image, H, W):
    return to_bytes(image_float(image, H, W))


def image_exact(image, H, W):
    """(C,H,W) float64: 255 times the interpolated value with the float32 weights and the exact u / 255"""
    return two_tap_float64(image, H, W)


def near_integer(exact, delta=DELTA):
    return np.abs(exact - np.rint(exact)) <= delta


def nearest_index(n_in, n_out):
    s = F32(n_in) / F32(n_out)
    return np.minimum(np.floor((np.arange(n_out, dtype=F32) * s).astype(F32)).astype(np.int64), n_in - 1)


def mask_nearest(mask, H, W):
    h, w = mask.shape
    return mask[nearest_index(h, H)][:, nearest_index(w, W)]


def K_resize(K, h, w, H, W):
    """get_K_crop_resize(K, box=(0, 0, w, h), orig_size=(h, w), crop_resize=(H, W)) in float32, in the reference's order"""
    K = np.asarray(K).astype(F32)
    new_K = K.copy()
    b0, b1, b2, b3 = F32(0), F32(0), F32(w), F32(h)
    final_width, final_height = F32(max(H, W)), F32(min(H, W))
    crop_width, crop_height = b2 - b0, b3 - b1
    crop_cj, crop_ci = (b0 + b2) / F32(2), (b1 + b3) / F32(2)
    cx = K[..., 0, 2] + (crop_width - F32(1)) / F32(2) - crop_cj
    cy = K[..., 1, 2] + (crop_height - F32(1)) / F32(2) - crop_ci
    center_x, center_y = (crop_width - F32(1)) / F32(2), (crop_height - F32(1)) / F32(2)
    orig_cx_diff, orig_cy_diff = cx - center_x, cy - center_y
    scale_x, scale_y = final_width / crop_width, final_height / crop_height
    scaled_center_x, scaled_center_y = (final_width - F32(1)) / F32(2), (final_height - F32(1)) / F32(2)
    new_K[..., 0, 0] = scale_x * K[..., 0, 0]
    new_K[..., 1, 1] = scale_y * K[..., 1, 1]
    new_K[..., 0, 2] = scaled_center_x + scale_x * orig_cx_diff
    new_K[..., 1, 2] = scaled_center_y + scale_y * orig_cy_diff
    assert new_K.dtype == F32
    return new_K


def instance_stats(mask, n_ids):
    """(n_ids,5) int32: count, x1, y1, x2, y2 per id, an absent id 0, -1, -1, -1, -1 (mask_ops.mask_instance_stats of one mask)"""
    out = np.full((n_ids, 5), -1, np.int32)
    out[:, 0] = 0
    for i in range(n_ids):
        ys, xs = np.where(mask == i)
        if len(ys):
            out[i] = len(ys), xs.min(), ys.min(), xs.max(), ys.max()
    return out


def resize_frame(image, resize, mask=None, K=None):
    """one frame of the right aspect -> dict(image (3,H,W) u8, mask (H,W) u8 | None, K (3,3) f32 | None, crop_resize_bbox 4 floats,
    resized bool)"""
    H, W = out_size(resize)
    C, h, w = image.shape
    if not np.isclose(w / h, W / H):
        raise ValueError(f'aspect {w / h} is not {W / H}')
    if (h, w) == (H, W):
        return dict(image=image.copy(), mask=None if mask is None else mask.copy(), K=None if K is None else np.asarray(K).astype(F32),
                    crop_resize_bbox=(0.0, 0.0, float(w - 1), float(h - 1)), resized=False)
    return dict(image=image_bytes(image, H, W), mask=None if mask is None else mask_nearest(mask, H, W),
                K=None if K is None else K_resize(K, h, w, H, W), crop_resize_bbox=(0.0, 0.0, float(w), float(h)), resized=True)


def parity_report(got, reference, exact):
    """the rule of section 18 for bytes `got` against the reference's: -> (bytes that differ outside the near-integer set, largest
    difference inside it, share of near-integer bytes)"""
    near = near_integer(exact)
    diff = np.abs(got.astype(np.int32) - reference.astype(np.int32))
    return int((diff[~near] != 0).sum()), int(diff[near].max()) if near.any() else 0, float(near.mean())

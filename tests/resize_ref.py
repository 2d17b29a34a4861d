"""numpy twin of cosypose_amd.resize.resize_images: Pillow 12's Image.resize of 8-bit images with BILINEAR and
BICUBIC, restated rule by rule -- the coefficient tables in double (plain Python floats: one rounding per operation, the sum of the
weights taken in index order), the two integer passes with the horizontal result rounded to bytes.  Test infrastructure, like
aug_ref.py: test_resize_host.py holds it against bytes recorded from Pillow (tests/golden/pillow_resize.npz) and against the library's
host routine, test_resize.py holds the kernels against it.  Images are (C,h,w) uint8 here; every channel is handled alike."""
import functools
import math

import numpy as np

BITS = 22
FILTERS = {'bilinear': 2, 'bicubic': 3}                      # Pillow's Image.BILINEAR, Image.BICUBIC = cosyhip.h: COSY_RESIZE_*
SUPPORT = {'bilinear': 1.0, 'bicubic': 2.0}


def bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTER_FN = {'bilinear': bilinear, 'bicubic': bicubic}


@functools.lru_cache(maxsize=None)
def coeffs(n_in, n_out, resample):
    """one axis -> bounds (n_out,2) int32 = xmin, xmax (first tap, number of taps) and k (n_out,ksize) int32 in 2^-22, zero past xmax"""
    f = FILTER_FN[resample]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds, k = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)           # int(): the C cast, toward zero
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:                                          # in index order, one addition at a time (numpy.sum adds pairwise)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(v * float(1 << BITS) - 0.5) if v < 0 else int(v * float(1 << BITS) + 0.5) for v in w]
        bounds[xx] = xmin, xmax
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def resample_last_axis(p, n_out, resample, raw=None):
    """(..., n_in) uint8 -> (..., n_out) uint8: 2^21 + the integer dot product, arithmetic shift by 22, clipped to a byte.  `raw`, when a
    list, receives the smallest and the largest value seen BEFORE the clip."""
    bounds, k = coeffs(p.shape[-1], n_out, resample)
    out = np.empty(p.shape[:-1] + (n_out,), np.uint8)
    q = p.astype(np.int64)
    for xx in range(n_out):
        a, n = (int(v) for v in bounds[xx])
        acc = (1 << (BITS - 1)) + (q[..., a:a + n] * k[xx, :n].astype(np.int64)).sum(axis=-1)
        assert np.abs(acc).max(initial=0) < 2 ** 31          # Pillow accumulates in int32
        if raw is not None and acc.size:
            raw += [int((acc >> BITS).min()), int((acc >> BITS).max())]
        out[..., xx] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(im, size, resample='bicubic', raw=None):
    """(C,h,w) uint8 -> (C,H,W) uint8, size = (H, W): rows first (skipped when W == w), rounded to bytes, then columns (skipped when
    H == h); an image already at size is copied"""
    H, W = size
    out = np.array(im, np.uint8)
    if W != out.shape[2]:
        out = resample_last_axis(out, W, resample, raw)
    if H != out.shape[1]:
        out = np.ascontiguousarray(resample_last_axis(out.transpose(0, 2, 1), H, resample, raw).transpose(0, 2, 1))
    return out


def resize_batch(images, size, resample='bicubic'):
    """list of (C,h_i,w_i) (or an (N,C,h,w) array) -> (N,C,H,W), the contract of resize_images"""
    C = images[0].shape[0] if len(images) else 3
    return np.stack([resize(im, size, resample) for im in images]) if len(images) else np.zeros((0, C) + tuple(size), np.uint8)


# ---- the recorded cases of tests/golden/pillow_resize.npz (tests/golden/generate_golden_resize.py) ----
def golden_cases(path):
    """-> {case: dict(images (n,C,h,w), size (H, W), contents [names], bilinear (n,C,H,W), bicubic (n,C,H,W))}, plus the raw arrays"""
    g = dict(np.load(path, allow_pickle=False))
    cases = {}
    for name in (str(c) for c in g['cases']):
        cases[name] = dict(images=g[f'{name}_images'], size=tuple(int(v) for v in g[f'{name}_size']), contents=[str(c) for c in g['contents']],
                           bilinear=g[f'{name}_bilinear'], bicubic=g[f'{name}_bicubic'])
    return cases, g

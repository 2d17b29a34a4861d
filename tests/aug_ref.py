"""numpy twin of the training augmentations: Pillow 12's GaussianBlur(k) and ImageEnhance Sharpness / Contrast /
Brightness / Color on uint8 RGB, the reference's float32 grey conversion and its background paste, restated rule by rule.  Test
infrastructure, like raster_ref.py: test_augmentations_host.py holds it against stage outputs recorded from Pillow, test_augmentations.py
holds the kernels against it.  Images are (H,W,3) uint8 here, as the reference's classes see them; `augment` also takes the (B,3,H,W)
batch and the parameter records of cosypose_amd.augmentations."""
import numpy as np

f32 = np.float32
BOX = {1: (0, 11184811, 2796202), 2: (1, 4473924, 1677722), 3: (2, 2876094, 1198373)}     # k -> r, ww, fw
STAGES = ('sharpness', 'contrast', 'brightness', 'color')


def clip8(t):
    """0 below 0, 255 above 255, else the C cast float -> UINT8 (truncation)"""
    t = np.asarray(t, f32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def luma(im):
    """convert('L')"""
    p = im.astype(np.uint32)
    return ((p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, im, f):
    """ImagingBlend(deg, im, f): product and sum each rounded to float32"""
    d = im.astype(np.int32) - deg.astype(np.int32)
    return clip8(deg.astype(f32) + f32(f) * d.astype(f32))


def box_pass(p, axis, r, ww, fw):
    """one box pass along `axis`, indices clamped to the line"""
    n = p.shape[axis]
    q = np.moveaxis(p, axis, 0).astype(np.uint32)
    at = lambda d: q[np.clip(np.arange(n) + d, 0, n - 1)]
    acc = sum(at(d) for d in range(-r, r + 1))
    far = at(-r - 1) + at(r + 1)
    out = (acc * np.uint32(ww) + far * np.uint32(fw) + np.uint32(1 << 23)) >> np.uint32(24)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def gaussian_blur(im, k):
    r, ww, fw = BOX[int(k)]
    for axis in (1, 0):                 # rows first (along x), then columns
        for _ in range(3):
            im = box_pass(im, axis, r, ww, fw)
    return im


def smooth(im):
    """ImageFilter.SMOOTH: (1,1,1,1,5,1,1,1,1)/13, the outermost rows and columns copied"""
    H, W = im.shape[:2]
    if H < 3 or W < 3:
        return im.copy()
    k1, k5 = f32(1) / f32(13), f32(5) / f32(13)
    p = im.astype(f32)
    row = lambda y, mid: (p[y, :-2] * k1 + p[y, 1:-1] * mid) + p[y, 2:] * k1
    ss = np.full((H - 2, W - 2, im.shape[2]), 0.5, f32)
    ss = ss + row(slice(2, H), k1)
    ss = ss + row(slice(1, H - 1), k5)
    ss = ss + row(slice(0, H - 2), k1)
    out = im.copy()
    out[1:-1, 1:-1] = clip8(ss)
    return out


def sharpness(im, f):
    return blend(smooth(im), im, f)


def contrast_mean(im):
    l = luma(im)
    return int((2 * int(l.sum(dtype=np.int64)) + l.size) // (2 * l.size))


def contrast(im, f):
    return blend(np.full_like(im, contrast_mean(im)), im, f)


def brightness(im, f):
    return blend(np.zeros_like(im), im, f)


def color(im, f):
    return blend(np.repeat(luma(im)[..., None], 3, axis=2), im, f)


def gray(im):
    p = im.astype(f32)
    g = (f32(0.2989) * p[..., 0] + f32(0.5870) * p[..., 1]) + f32(0.1140) * p[..., 2]
    return np.repeat(g.astype(np.uint8)[..., None], 3, axis=2)


def paste(im, mask, bg):
    out = im.copy()
    out[mask == 0] = bg[mask == 0]
    return out


ENHANCE = dict(sharpness=sharpness, contrast=contrast, brightness=brightness, color=color)


def augment_one(im, rec, mask=None, backgrounds=None, stages=None):
    """(H,W,3) uint8 through the chain described by the record `rec` (a dict as cosypose_amd.augmentations.draw_sample_params returns).
    `stages`, when a list, receives (name, image) after every stage that ran."""
    note = (lambda n, v: stages.append((n, v))) if stages is not None else (lambda n, v: None)
    if rec['bg'] >= 0:
        im = paste(im, mask, np.ascontiguousarray(backgrounds[rec['bg']].transpose(1, 2, 0)))
        note('background', im)
    if not rec['gate']:
        return im
    im = gaussian_blur(im, rec['k'])
    note('blur', im)
    for name in STAGES:
        if rec[name] is not None:
            im = ENHANCE[name](im, rec[name])
            note(name, im)
    if rec['gray']:
        im = gray(im)
        note('gray', im)
    return im


def augment(images, recs, masks=None, backgrounds=None):
    """(B,3,H,W) uint8 -> (B,3,H,W) uint8, the contract of cosypose_amd.augmentations.augment_batch"""
    out = [augment_one(np.ascontiguousarray(im.transpose(1, 2, 0)), rec, None if masks is None else masks[b], backgrounds)
           for b, (im, rec) in enumerate(zip(images, recs))]
    return np.stack([o.transpose(2, 0, 1) for o in out]) if out else images.copy()


# ---- the recorded cases of tests/golden/reference_golden_aug.npz (tests/golden/generate_golden_aug.py) ----
def record_from_row(row, fields):
    """a row of <case>_rec -> the record dict of cosypose_amd.augmentations (NaN = stage skipped)"""
    r = dict(zip(fields, row))
    rec = dict(bg=int(r['bg']), gate=bool(r['gate']), k=int(r['k']), gray=bool(r['gray']))
    for name in STAGES:
        rec[name] = None if np.isnan(r[name]) else float(r[name])
    return rec


def golden_cases(path):
    """-> {case: dict(images, masks, backgrounds, recs, out, stages={stage: (indices, images)})}, plus the raw arrays"""
    g = dict(np.load(path, allow_pickle=False))
    fields = [str(f) for f in g['rec_fields']]
    cases = {}
    for name in [f'seed{s}' for s in g['seeds']] + [str(c) for c in g['forced_cases']]:
        cases[name] = dict(images=g[f'{name}_images'], masks=g[f'{name}_masks'], backgrounds=g[f'{name}_backgrounds'], out=g[f'{name}_out'],
                           recs=[record_from_row(row, fields) for row in g[f'{name}_rec']],
                           stages={str(st): (g[f'{name}_stage_{st}_idx'], g[f'{name}_stage_{st}']) for st in g['stage_names']
                                   if f'{name}_stage_{st}' in g})
    return cases, g

"""Inputs of test_image_kernels.py (GPU) and test_image_kernels_host.py (CPU): the image kernels -- augmentations (kernels_aug.hip),
Pillow resize (kernels_resize.hip), the frames' own resize (kernels_frames.hip) -- over the full byte range and at the edges of their
tiles.  Plain numpy on top of the twins aug_ref / resize_ref / frames_ref; nothing here imports cosypose_amd or torch.  Both test files
build their inputs here, so the coverage conditions that the host file proves on the twins hold for the very bytes the GPU file runs.
Everything is seeded; builders are cached and hand out read-only arrays."""
import functools

import numpy as np

import aug_ref
import resize_ref

BLOCK = 20                                                   # block edge: three box passes of GaussianBlur(3) reach 9 pixels
FILTERS = ('bilinear', 'bicubic')
NO_STAGE = dict(sharpness=None, contrast=None, brightness=None, color=None)


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def rec(k, gray=False, bg=-1, **stages):
    """a record as cosypose_amd.augmentations.draw_sample_params returns it, gate on"""
    assert set(stages) <= set(NO_STAGE)
    return dict(NO_STAGE, bg=bg, gate=True, k=k, gray=gray, **stages)


def hwc(im):
    return np.ascontiguousarray(im.transpose(1, 2, 0))


# ---------------------------------------------------------------- A1: block images
@functools.lru_cache(maxsize=None)
def values256():
    """(3,320,320): 16x16 blocks of 20x20; channel 0 holds every byte value in block order, channels 1 and 2 seeded permutations of them.
    -> image, colours (256,3) in block order"""
    rs = np.random.RandomState(256)
    colours = np.stack([np.arange(256), rs.permutation(256), rs.permutation(256)], axis=1).astype(np.uint8)
    return frozen(blocks_image(colours, 16)), frozen(colours)


@functools.lru_cache(maxsize=None)
def colours4096():
    """(3,1280,1280): 64x64 blocks, every combination of the 16 levels 0, 17, .., 255 per channel, in seeded order"""
    levels = np.arange(16) * 17
    colours = np.stack(np.meshgrid(levels, levels, levels, indexing='ij'), axis=-1).reshape(-1, 3).astype(np.uint8)
    colours = colours[np.random.RandomState(4096).permutation(len(colours))]
    return frozen(blocks_image(colours, 64)), frozen(colours)


def blocks_image(colours, side):
    grid = colours.reshape(side, side, 3).transpose(2, 0, 1)
    return np.repeat(np.repeat(grid, BLOCK, axis=1), BLOCK, axis=2)


def block_centres(image, side):
    """(3,H,W) -> (side*side,3): the two central pixels of every block along the diagonal must agree; returns the one at offset 10"""
    c = np.arange(side) * BLOCK + BLOCK // 2
    at = image[:, c][:, :, c]
    assert np.array_equal(at, image[:, c - 1][:, :, c - 1])
    return at.transpose(1, 2, 0).reshape(-1, 3)


SINGLE_FACTORS = (('sharpness', (0., 1., 7.5, 50.)), ('contrast', (0.2, 1., 3., 50.)), ('brightness', (0.1, 1., 1.5, 6.)), ('color', (0., 1., 4., 20.)))
GRAY_AFTER = dict(sharpness=7.5, contrast=3., brightness=1.5, color=4.)


@functools.lru_cache(maxsize=None)
def single_stage_records():
    """one record per (stage, factor) with only that stage on after the blur, grey alone, grey after each of the other stages; k cycles
    over 1..3.  -> list of (label, record)"""
    out = []
    for name, factors in SINGLE_FACTORS:
        out += [(f'{name}={f}', {name: f}, False) for f in factors]
    out.append(('gray', {}, True))
    out += [(f'{name}={f}+gray', {name: f}, True) for name, f in GRAY_AFTER.items()]
    return tuple((label, rec(1 + i % 3, gray=gray, **stages)) for i, (label, stages, gray) in enumerate(out))


def full_chain_records():
    """all stages on, k = 1, 2, 3, factors from the middle of the reference's ranges (the midpoint, the first and the third quartile)"""
    ranges = dict(sharpness=(0., 50.), contrast=(0.2, 50.), brightness=(0.1, 6.), color=(0., 20.))
    at = lambda q: {name: lo + q * (hi - lo) for name, (lo, hi) in ranges.items()}
    return [rec(1, **at(0.5)), rec(2, gray=True, **at(0.25)), rec(3, **at(0.75))]


def blend_clip_shares(deg, im, f):
    """the shares of bytes that ImagingBlend's two clip branches take: t <= 0 and t >= 255 with t = deg + f (im - deg) in float32"""
    t = deg.astype(np.float32) + np.float32(f) * (im.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    return float((t <= 0).mean()), float((t >= 255).mean())


def constant_frames(h, w):
    """(256,3,h,w): frame v is the constant v; with them the records of A1's constant test (k cycles, nothing else on / sharpness 2)"""
    images = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 3, h, w))
    plain = [rec(1 + v % 3) for v in range(256)]
    sharp = [rec(1 + v % 3, sharpness=2.0) for v in range(256)]
    return frozen(images), plain, sharp


# ---------------------------------------------------------------- A2: tile edges
# exact multiples and remainders of 1, 9 and 10 of the row tiles (8x128, halo 9) and the column tiles (64x64, halo 10 rows, 1 column)
AUG_EDGE_SIZES = ((7, 127), (8, 128), (9, 129), (16, 137), (17, 138), (63, 63), (64, 64), (65, 65), (74, 66), (75, 67), (128, 256))
SEAM_COLUMNS, SEAM_ROWS = (127, 128), (7, 8, 63, 64)


def seam_frame(h, w):
    """(3,h,w): zero but for 255 on the columns and rows that straddle the tile borders, wherever they exist"""
    im = np.zeros((3, h, w), np.uint8)
    im[:, :, [x for x in SEAM_COLUMNS if x < w]] = 255
    im[:, [y for y in SEAM_ROWS if y < h]] = 255
    return im


@functools.lru_cache(maxsize=None)
def aug_edge_batch(h, w):
    """-> images (8,3,h,w), masks (8,h,w), backgrounds (2,3,h,w), records: the 0/255 noise frame and the seam frame, each with k = 3 and
    sharpness and with k = 1 and nothing else, each with and without the paste from a background"""
    rs = np.random.RandomState(h * 1000 + w)
    noise = (rs.randint(0, 2, (3, h, w)) * 255).astype(np.uint8)
    frames, recs = [], []
    for paste in (False, True):
        for im in (noise, seam_frame(h, w)):
            for k, stages in ((3, dict(sharpness=7.5)), (1, {})):
                frames.append(im)
                recs.append(rec(k, bg=len(recs) % 2 if paste else -1, **stages))
    masks = (rs.rand(len(frames), h, w) < 0.5).astype(np.uint8) * 5
    backgrounds = rs.randint(0, 256, (2, 3, h, w)).astype(np.uint8)
    return frozen(np.stack(frames)), frozen(masks), frozen(backgrounds), recs


# ---------------------------------------------------------------- A3: Contrast's mean
def blurred_l_sum(image, k=1):
    """(3,h,w) -> (sum of L over the frame Contrast sees with sharpness off, number of pixels)"""
    l = aug_ref.luma(aug_ref.gaussian_blur(hwc(image), k))
    return int(l.sum(dtype=np.int64)), l.size


@functools.lru_cache(maxsize=None)
def tie_frames(want=4, candidates=400):
    """small frames (up to 4x4) whose blurred mean L is an exact tie, (2 sum + n) % (2 n) == 0, with different means.
    -> list of (image (3,h,w), mean)"""
    rs = np.random.RandomState(43)
    sizes = ((1, 2), (2, 2), (2, 3), (3, 4), (4, 4), (4, 3), (2, 1), (3, 2))
    found, means = [], set()
    for i in range(candidates):
        h, w = sizes[i % len(sizes)]
        image = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
        s, n = blurred_l_sum(image)
        mean = (2 * s + n) // (2 * n)
        if (2 * s + n) % (2 * n) == 0 and mean not in means and (h, w) not in {f.shape[1:] for f, _ in found}:
            found.append((frozen(image), mean))
            means.add(mean)
            if len(found) == want:
                break
    return found


@functools.lru_cache(maxsize=None)
def mean_range_frames(h=9, w=12, candidates=400):
    """one frame each whose twin mean is 0 (with a sum above 0), 1, 254 and 255 (with a sum below 255 n) -> {mean: image (3,h,w)}"""
    rs = np.random.RandomState(254)
    found = {}
    for i in range(candidates):
        base = 0 if i % 2 == 0 else 255
        image = np.full((3, h, w), base, np.uint8)
        n_px = rs.randint(1, h * w // 2)
        ys, xs = rs.randint(0, h, n_px), rs.randint(0, w, n_px)
        image[:, ys, xs] = np.abs(base - rs.randint(1, 9, (3, n_px))).astype(np.uint8)
        s, n = blurred_l_sum(image)
        mean = (2 * s + n) // (2 * n)
        if mean in (0, 1, 254, 255) and mean not in found and 0 < s < 255 * n:
            found[mean] = frozen(image)
        if len(found) == 4:
            break
    return found


HALF_SIZES = ((8, 128), (64, 64), (64, 128), (128, 128))     # one row tile, one column tile, two, four


def half_frame(h, w, vertical):
    """(3,h,w): one half 0, the other 255, split along x or along y"""
    im = np.zeros((3, h, w), np.uint8)
    if vertical:
        im[:, :, w // 2:] = 255
    else:
        im[:, h // 2:] = 255
    return im


CONTRAST_FACTORS = (0.2, 3.0, 50.0)


# ---------------------------------------------------------------- B1: the resize accumulator at its extremes
RESIZE_AXES = ((7, 5), (211, 32), (300, 6), (3, 300), (257, 256), (2000, 1), (1, 9))


@functools.lru_cache(maxsize=None)
def tap_sign_lines(n_in, n_out, resample):
    """the two source lines that drive one axis's accumulator furthest: 255 where the taps of the output index with the largest sum of
    positive taps are positive, and 255 where the taps of the index with the most negative sum of negative taps are negative.
    -> dict(pos, neg: (n_in,) uint8; xx_pos, xx_neg: the indices; acc_pos, acc_neg: their accumulators in Python ints)"""
    bounds, k = resize_ref.coeffs(n_in, n_out, resample)
    k64 = k.astype(np.int64)
    xx_pos = int(np.where(k64 > 0, k64, 0).sum(axis=1).argmax())
    xx_neg = int(np.where(k64 < 0, k64, 0).sum(axis=1).argmin())
    out = dict(xx_pos=xx_pos, xx_neg=xx_neg)
    for name, xx, sign in (('pos', xx_pos, 1), ('neg', xx_neg, -1)):
        a, n = (int(v) for v in bounds[xx])
        line = np.zeros(n_in, np.uint8)
        line[a:a + n][sign * k64[xx, :n] > 0] = 255
        out[name] = frozen(line)
        out['acc_' + name] = (1 << (resize_ref.BITS - 1)) + sum(int(p) * int(c) for p, c in zip(line[a:a + n], k64[xx, :n]))
    return out


def tap_sign_image(n_in, n_out, resample):
    """(3,5,n_in): the rows pos, neg, 255 - pos, 255 - neg, pos, rolled by one row from plane to plane; rows 0 and 1 of plane 0 are the two
    extreme lines.  Its transpose (3,n_in,5) meets the same accumulators in the vertical pass."""
    t = tap_sign_lines(n_in, n_out, resample)
    rows = np.stack([t['pos'], t['neg'], 255 - t['pos'], 255 - t['neg'], t['pos']])
    return np.stack([np.roll(rows, c, axis=0) for c in range(3)])


# ---------------------------------------------------------------- B2: constants through the resize
# each of the ratios 7->5, 5->7, 211->32 and 3->300 on each axis: (h, w, H, W)
RESIZE_CONSTANT_SHAPES = ((3, 5, 300, 7), (5, 3, 7, 300), (7, 211, 5, 32), (211, 7, 32, 5))


def constant_images(h, w):
    """(256,1,h,w): image v is the constant v"""
    return frozen(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 1, h, w)))


# ---------------------------------------------------------------- B3: resize tile edges (4 rows x 256 bytes) and one-pixel axes
RESIZE_EDGE_WIDTHS, RESIZE_EDGE_HEIGHTS = (1, 3, 4, 5, 255, 256, 257, 260), (1, 3, 4, 5)
RESIZE_EDGE_SOURCES = ((6, 261), (11, 31))
# 8001 bicubic taps on one axis, and a frame down to one pixel
RESIZE_LONG_SHAPES = ((2000, 3, 1, 3), (3, 2000, 3, 1), (97, 211, 1, 1))


def resize_edge_shapes():
    """(h, w, H, W, byte offset of `out`): every output width with every output height, the sources and the offsets 0..3 taking turns"""
    out = []
    for iw, W in enumerate(RESIZE_EDGE_WIDTHS):
        for ih, H in enumerate(RESIZE_EDGE_HEIGHTS):
            h, w = RESIZE_EDGE_SOURCES[(iw + ih // 2) % 2]
            out.append((h, w, H, W, (iw + ih) % 4))
    return out + [s + (1 + i,) for i, s in enumerate(RESIZE_LONG_SHAPES)]


def resize_edge_images(h, w, C):
    """(2,C,h,w): seeded noise and a seeded 0/255 image"""
    rs = np.random.RandomState(h * 10000 + w * 10 + C)
    return frozen(np.stack([rs.randint(0, 256, (C, h, w)), rs.randint(0, 2, (C, h, w)) * 255]).astype(np.uint8))


# ---------------------------------------------------------------- C1: frames, every byte value and the two-level extremes
# the first three have dyadic weights (1/2, 1/4, 3/4): l0 p + l1 p is p exactly; the last two (scales 2/3 and 5/3) round in every step
FRAME_CONSTANT_SHAPES = ((6, 8, 3, 4), (9, 12, 6, 8), (3, 4, 12, 16), (6, 8, 9, 12), (15, 20, 9, 12))
FRAME_STRUCTURED_SHAPES = ((96, 128, 48, 64), (99, 132, 93, 124), (33, 44, 99, 132))


def frame_constants(h, w):
    """-> images (256,3,h,w), frame v the constant v; masks (256,h,w), mask v = (v + y w + x) % 256: together they hold every id"""
    images = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 3, h, w))
    masks = (np.arange(256)[:, None, None] + ramp(h, w)[None]) % 256
    return frozen(images), frozen(masks.astype(np.uint8))


def ramp(h, w):
    return ((np.arange(h)[:, None] * w + np.arange(w)[None, :]) % 256).astype(np.uint8)


def frame_structured(h, w):
    """-> images (2,3,h,w): a 0/255 checkerboard (shifted by one pixel from plane to plane) and the ramp (y w + x) % 256 (offset by 85 per
    plane); masks (2,h,w): the ramp and its mirror image, every id 0..255 where the frame has 256 pixels"""
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    checker = np.stack([((yy + xx + c) % 2 * 255) for c in range(3)])
    ramps = np.stack([(ramp(h, w).astype(np.int64) + 85 * c) % 256 for c in range(3)])
    masks = np.stack([ramp(h, w), ramp(h, w)[::-1, ::-1]])
    return frozen(np.stack([checker, ramps]).astype(np.uint8)), frozen(masks)


# ---------------------------------------------------------------- C2: frames tile edges (8 rows x 128 bytes) and odd addresses
# (H, W) -> the up-scaling and the down-scaling source (h, w), all of aspect 4:3
FRAME_EDGE_SHAPES = {(93, 124): ((33, 44), (150, 200)), (96, 128): ((33, 44), (150, 200)), (99, 132): ((33, 44), (150, 200)),
                     (192, 256): ((99, 132), (240, 320))}


def frame_edge_inputs(h, w):
    """-> images (2,3,h,w): seeded noise and the seam frame; masks (2,h,w): seeded ids and the ramp"""
    rs = np.random.RandomState(h * 1000 + w)
    images = np.stack([rs.randint(0, 256, (3, h, w)).astype(np.uint8), seam_frame(h, w)])
    masks = np.stack([rs.randint(0, 256, (h, w)).astype(np.uint8), ramp(h, w)])
    return frozen(images), frozen(masks)

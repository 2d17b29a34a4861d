#!/usr/bin/env python3
"""Writes tests/golden/pillow_resize.npz: what Pillow's Image.resize gives, with BILINEAR and with BICUBIC, on small 8-bit images.
Pillow only; nothing else is involved.  The committed file was written under Pillow 12.2.0 (`pil_version` inside), the version whose
bytes DESIGN.md sections 14 and 17 are pinned to.

    python tests/golden/generate_golden_resize.py

Per case `<h>x<w>_to_<H>x<W>[_c1]`: `_images` (4,C,h,w) uint8, one image per entry of `contents` (random bytes, constant 0, constant
255, a 0/255 checkerboard of squares a few output pixels wide: under bicubic its edges overshoot both clips); `_size` = (H, W);
`_bilinear`, `_bicubic` (4,C,H,W) uint8.  C = 3 is an RGB image, C = 1 an L image.  The script also checks what section 17 rests on: resize without a filter IS the bicubic one, and
an image already at size comes back as an equal copy."""
import pathlib

import numpy as np
import PIL
from PIL import Image

# h, w, H, W
SHAPES = ((1, 1, 4, 5),          # every tap clamped from both sides
          (2, 3, 5, 7),          # small upscale
          (3, 2, 1, 1),          # window wider than the image
          (5, 7, 5, 9),          # horizontal pass only
          (5, 7, 8, 7),          # vertical pass only
          (24, 32, 24, 32),      # copy
          (37, 53, 48, 64),      # the VOC-like upscale ratio
          (97, 211, 24, 32),     # downscale by 4 and 6.6, up to 29 taps
          (131, 67, 70, 150),    # down in one axis and up in the other, several tiles each way
          (300, 8, 6, 8))        # factor 50
C1 = ((37, 53, 48, 64), (131, 67, 70, 150))
CONTENTS = ('random', 'zeros', 'ones', 'checkerboard')


def make_images(rs, C, h, w, H, W):
    y, x = np.mgrid[0:h, 0:w]
    cell = 3 * int(np.ceil(max(h / H, w / W, 1.0)))          # squares that survive the downscale: their edges overshoot
    board = (((x // cell + y // cell) % 2) * 255).astype(np.uint8)
    return np.stack([rs.randint(0, 256, (C, h, w)).astype(np.uint8), np.zeros((C, h, w), np.uint8), np.full((C, h, w), 255, np.uint8),
                     np.repeat(board[None], C, axis=0)])


def to_pil(im):
    return Image.fromarray(im[0], 'L') if im.shape[0] == 1 else Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0)), 'RGB')


def from_pil(pil):
    a = np.asarray(pil)
    return a[None].copy() if a.ndim == 2 else np.ascontiguousarray(a.transpose(2, 0, 1))


def main():
    rs = np.random.RandomState(20261018)
    out = dict(pil_version=np.array(PIL.__version__), contents=np.array(CONTENTS))
    names = []
    for C, shapes in ((3, SHAPES), (1, C1)):
        for h, w, H, W in shapes:
            name = f'{h}x{w}_to_{H}x{W}' + ('_c1' if C == 1 else '')
            names.append(name)
            images = make_images(rs, C, h, w, H, W)
            out[f'{name}_images'], out[f'{name}_size'] = images, np.array([H, W], np.int32)
            for key, filt in (('bilinear', Image.BILINEAR), ('bicubic', Image.BICUBIC)):
                out[f'{name}_{key}'] = np.stack([from_pil(to_pil(im).resize((W, H), filt)) for im in images])
            default = np.stack([from_pil(to_pil(im).resize((W, H))) for im in images])
            assert np.array_equal(default, out[f'{name}_bicubic']), name         # the default filter of RGB and L images is BICUBIC
            if (h, w) == (H, W):
                assert np.array_equal(default, images), name
    out['cases'] = np.array(names)
    path = pathlib.Path(__file__).resolve().parent / 'pillow_resize.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes,', len(names), 'cases, Pillow', PIL.__version__)


if __name__ == '__main__':
    main()

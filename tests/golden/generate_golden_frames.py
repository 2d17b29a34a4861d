#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_frames.npz: the REFERENCE's own CropResizeToAspectAugmentation.__call__ (cosypose/datasets/
augmentations.py:137-192), run in place on seeded frames of the target aspect -- the step that brings every frame of PoseDataset and
DetectionDataset to the training size.  Run in the build container only:
    python tests/golden/generate_golden_frames.py

Shims as in generate_golden_aug.py: generate_golden.install_stubs and an empty torchvision.datasets.ImageFolder.  torch runs on ONE
thread, as in the other generators; with three channels and one thread torch takes its vectorised channels-last kernel, so at the pixels
whose exact value is an integer the bytes stored here may lie one level off DESIGN.md section 18's definition (which is torch's generic
kernel): the tests hold them to section 18's parity rule, not to equality.

Per case `<h>x<w>_to_<H>x<W>`: `_image` (3,h,w) uint8 random bytes, `_mask` (h,w) uint8 with ids 0..5 of which id ABSENT_ID owns no
pixel and id 1 touches the border, `_K` (3,3) float64, `_resize` the (2,) argument of the class; `_out_image` (3,H,W), `_out_mask`
(H,W), `_out_K` (3,3) as the reference leaves it, `_bbox` (4,) float64 = orig_camera['crop_resize_bbox'], `_boxes` (N_IDS,4) int64 =
the refreshed obj['bbox'] of the object with that id_in_segm (the absent id carries no 'bbox', as an object without a pixel must: the
reference would raise a KeyError for it; its row is -1), `_resized` 0 / 1.  For the frame already at size the boxes are the ones handed
in (-7 everywhere): the reference returns early and leaves them.

For every resized case the share of bytes whose float64-exact value lies within 1e-4 of an integer is asserted to be at most 1 %.
"""
import sys
import types
import pathlib

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import numpy as np
import torch

import generate_golden as gg
from generate_golden_ba import save_npz
import frames_ref

OUT = HERE / 'reference_golden_frames.npz'
# h, w, resize argument (the class sorts it: (H, W) = (min, max))
CASES = ((99, 132, (64, 48)), (45, 60, (64, 48)), (54, 72, (64, 48)), (150, 200, (128, 96)), (50, 50, (32, 32)), (48, 64, (64, 48)))
N_IDS, ABSENT_ID = 6, 4
MAX_NEAR_SHARE = 0.01


def reference():
    gg.install_stubs()
    ds = types.ModuleType('torchvision.datasets')
    ds.ImageFolder = type('ImageFolder', (), {})
    sys.modules['torchvision.datasets'] = ds
    sys.modules['torchvision'].datasets = ds
    from cosypose.datasets import augmentations as A
    return A


def make_mask(rs, h, w):
    """ids 0..5 without ABSENT_ID: rectangles at least a sixth of the frame in each direction (they survive every downscale here), id 1
    in the top left corner, so its box touches the border"""
    m = np.zeros((h, w), np.uint8)
    for i in range(1, N_IDS):
        if i == ABSENT_ID:
            continue
        hh, ww = rs.randint(h // 6 + 1, h // 2 + 1), rs.randint(w // 6 + 1, w // 2 + 1)
        y0, x0 = (0, 0) if i == 1 else (rs.randint(0, h - hh + 1), rs.randint(0, w - ww + 1))
        m[y0:y0 + hh, x0:x0 + ww] = i
    m[0, 0] = 1
    assert set(np.unique(m)) <= set(range(N_IDS)) and ABSENT_ID not in m
    return m


def main():
    A = reference()
    torch.set_num_threads(1)
    rs = np.random.RandomState(20261019)
    arrays, names = {}, []
    for h, w, resize in CASES:
        H, W = frames_ref.out_size(resize)
        name = f'{h}x{w}_to_{H}x{W}'
        names.append(name)
        image = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
        mask = make_mask(rs, h, w)
        K = np.array([[rs.uniform(0.8, 1.6) * w, 0.0, w / 2 + rs.uniform(-5, 5)], [0.0, rs.uniform(0.8, 1.6) * w, h / 2 + rs.uniform(-5, 5)],
                      [0.0, 0.0, 1.0]])
        present = [i for i in range(N_IDS) if (mask == i).any()]
        objects = [dict(id_in_segm=i, bbox=np.full(4, -7)) if i in present else dict(id_in_segm=i) for i in range(N_IDS)]
        obs = dict(camera=dict(K=K.copy(), resolution=(w, h)), objects=objects)
        im_out, mask_out, obs_out = A.CropResizeToAspectAugmentation(resize=resize)(np.ascontiguousarray(image.transpose(1, 2, 0)), mask.copy(), obs)
        im_out, mask_out = np.asarray(im_out), np.asarray(mask_out)
        assert im_out.shape == (H, W, 3) and im_out.dtype == np.uint8 and mask_out.shape == (H, W) and mask_out.dtype == np.uint8, name
        resized = (h, w) != (H, W)
        boxes = np.full((N_IDS, 4), -1, np.int64)
        for obj in obs_out['objects']:
            if 'bbox' in obj:
                boxes[obj['id_in_segm']] = np.asarray(obj['bbox'])
        arrays[f'{name}_image'], arrays[f'{name}_mask'], arrays[f'{name}_K'] = image, mask, K
        arrays[f'{name}_resize'] = np.array(resize, np.int32)
        arrays[f'{name}_out_image'] = np.ascontiguousarray(im_out.transpose(2, 0, 1))
        arrays[f'{name}_out_mask'] = mask_out
        arrays[f'{name}_out_K'] = np.asarray(obs_out['camera']['K'])
        arrays[f'{name}_bbox'] = np.array(obs_out['orig_camera']['crop_resize_bbox'], np.float64)
        arrays[f'{name}_boxes'] = boxes
        arrays[f'{name}_resized'] = np.array(int(resized), np.int32)
        if resized:
            assert sorted(np.unique(mask_out)) == present, (name, 'an id vanished in the downscale')
            share = float(frames_ref.near_integer(frames_ref.image_exact(image, H, W)).mean())
            assert share <= MAX_NEAR_SHARE, (name, share)
            print(f'{name}: near-integer share {100 * share:.3f} %')
    arrays['cases'] = np.array(names)
    arrays['n_ids'], arrays['absent_id'] = np.array(N_IDS, np.int32), np.array(ABSENT_ID, np.int32)
    arrays['torch_version'] = np.array(torch.__version__)
    save_npz(OUT, arrays)
    print('wrote', OUT, OUT.stat().st_size, 'bytes; torch', torch.__version__)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_aug.npz: the REFERENCE's own augmentation classes (cosypose/datasets/augmentations.py:
BackgroundAugmentation.__call__, PillowBlur, PillowSharpness, PillowContrast, PillowBrightness, PillowColor, GrayScale), run in place
with Pillow, in the order and under the gate of PoseDataset.get_data (pose_dataset.py:82-87).  Run in the build container only:
    python tests/golden/generate_golden_aug.py

Shims, next to generate_golden.install_stubs: an empty torchvision.datasets.ImageFolder (augmentations.py:6 imports it; only
VOCBackgroundAugmentation, which is not run, uses it).  get_data itself needs a scene dataset and VOC on disk; its three lines that
matter here -- background, `random.random() < 0.8`, the loop over rgb_augmentations -- are restated in chain().

The classes read the module-level name `random`.  It is replaced by a recorder that either passes the calls on to Python's global
generator (seeded runs: the draws are the reference's own, and are recorded) or answers them from a script (forced cases: 0.0 takes a
stage, 1.0 skips it, the factor / k / background row are the ones the case names).  A sample's parameter record is read off the draws
each class made, not computed: a `uniform` after a stage's `random` is that stage's factor.

Two kinds of case, each a batch of equal frames (forced_cases() says why each exists):
  seed<s>   random.seed(s), then N_SEEDED samples of SEEDED_HW with background, rgb and gray augmentation all enabled; also recorded:
            every draw (kind, value) per sample, and the next random.random() after the last sample;
  forced    fixed records on frames of 1x1, 2x3, 3x3, 5x7, 37x53, 48x64 and 67x131.
Recorded per case: images, masks, backgrounds, records, the output, and the image after every stage that ran (with the indices of the
images it ran on), plus PIL.__version__.
"""
import random
import sys
import types
import pathlib

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import numpy as np
import PIL
import torch

import generate_golden as gg
from generate_golden_ba import save_npz

OUT = HERE / 'reference_golden_aug.npz'
SEEDS = (0, 1, 2, 3)
N_SEEDED, SEEDED_HW, N_BG = 6, (24, 32), 3
STAGE_NAMES = ('background', 'blur', 'sharpness', 'contrast', 'brightness', 'color', 'gray')
KIND = {'random': 0, 'randint': 1, 'uniform': 2}
MAX_DRAWS = 16
REC_FIELDS = ('bg', 'gate', 'k', 'sharpness', 'contrast', 'brightness', 'color', 'gray')     # columns of <case>_rec, NaN = stage skipped
# The device kernels work on 8 x 128 (rows) and 64 x 64 (columns) tiles: 67 x 131 exceeds both, in both directions, by 3.
BIG_HW = (67, 131)


class Recorder:
    """stands in for the `random` module inside the reference's augmentations.py"""

    def __init__(self):
        self.log, self.script = [], None

    def _draw(self, kind, *args):
        v = self.script.pop(0) if self.script is not None else getattr(random, kind)(*args)
        self.log.append((kind, v))
        return v

    def random(self):
        return self._draw('random')

    def randint(self, a, b):
        v = self._draw('randint', a, b)
        assert a <= v <= b
        return v

    def uniform(self, a, b):
        return self._draw('uniform', a, b)


def reference():
    gg.install_stubs()
    ds = types.ModuleType('torchvision.datasets')
    ds.ImageFolder = type('ImageFolder', (), {})
    sys.modules['torchvision.datasets'] = ds
    sys.modules['torchvision'].datasets = ds
    from cosypose.datasets import augmentations as A
    rec = Recorder()
    A.random = rec
    return A, rec


def make_frame(rs, H, W, kind='mixed'):
    """structured and random content: gradients, a few rectangles with hard edges, noise on a part of the frame"""
    if kind == 'random':
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    im = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 37) % 256], -1).astype(np.int32)
    for _ in range(4):
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        im[y0:y0 + rs.randint(1, max(H // 2, 2)), x0:x0 + rs.randint(1, max(W // 2, 2))] = rs.randint(0, 256, 3)
    noisy = x >= W // 2
    im[noisy] += rs.randint(-40, 41, (int(noisy.sum()), 3))
    return np.clip(im, 0, 255).astype(np.uint8)


def make_mask(rs, H, W, kind):
    if kind == 'zero':
        return np.zeros((H, W), np.uint8)
    if kind == 'full':
        return rs.randint(1, 5, (H, W)).astype(np.uint8)
    m = np.zeros((H, W), np.uint8)
    m[H // 4:H - H // 4, W // 3:] = 2
    m[rs.rand(H, W) < 0.1] = 1
    return m


def chain(A, rec, im, mask, backgrounds, background_augmentation, rgb_augmentation, gray_augmentation):
    """pose_dataset.py:82-87 on one sample with the reference's classes -> final image, record, {stage: image}"""
    to_np = lambda v: np.array(A.to_torch_uint8(v))
    augs = [A.PillowBlur(p=0.4, factor_interval=(1, 3)), A.PillowSharpness(p=0.3, factor_interval=(0., 50.)),
            A.PillowContrast(p=0.3, factor_interval=(0.2, 50.)), A.PillowBrightness(p=0.5, factor_interval=(0.1, 6.0)),
            A.PillowColor(p=0.3, factor_interval=(0., 20.))]
    if gray_augmentation:
        augs.append(A.GrayScale(p=0.5))
    out = dict(bg=-1, gate=0, k=0, sharpness=np.nan, contrast=np.nan, brightness=np.nan, color=np.nan, gray=0)
    stages, state = {}, {}
    rgb, mask = im.copy(), mask.copy()
    if background_augmentation:
        n0 = len(rec.log)
        rgb, mask, state = A.BackgroundAugmentation([b.transpose(1, 2, 0).copy() for b in backgrounds], p=0.3)(rgb, mask, state)
        drawn = rec.log[n0:]
        if len(drawn) == 2:
            out['bg'] = drawn[1][1]
            stages['background'] = to_np(rgb)
    if rgb_augmentation and rec.random() < 0.8:
        out['gate'] = 1
        for name, aug in zip(STAGE_NAMES[1:], augs):
            n0 = len(rec.log)
            rgb, mask, state = aug(rgb, mask, state)
            drawn = rec.log[n0:]
            if name == 'blur':
                assert [d[0] for d in drawn] == ['randint']
                out['k'] = drawn[0][1]
            elif name == 'gray':
                assert [d[0] for d in drawn] == ['random']
                out['gray'] = int(drawn[0][1] <= 0.5)
                if not out['gray']:
                    continue
            else:
                assert [d[0] for d in drawn] in (['random'], ['random', 'uniform'])
                if len(drawn) == 1:
                    continue
                out[name] = drawn[1][1]
            stages[name] = to_np(rgb)
    return to_np(rgb), out, stages


def script_for(r, background_augmentation, gray_augmentation):
    """the answers that make the classes follow record r"""
    s = []
    if background_augmentation:
        s += [0.0, r['bg']] if r['bg'] >= 0 else [1.0]
    s.append(0.0 if r['gate'] else 0.9)
    if r['gate']:
        s.append(r['k'])
        for name in STAGE_NAMES[2:6]:
            s += [0.0, r[name]] if r.get(name) is not None else [1.0]
        if gray_augmentation:
            s.append(0.0 if r.get('gray') else 1.0)
    return s


def R(k=1, bg=-1, gate=1, gray=0, **factors):
    return dict(bg=bg, gate=gate, k=k, gray=gray, **factors)


ALL = dict(sharpness=7.3, contrast=1.9, brightness=1.4, color=2.6)


def forced_cases(A, rec):
    """name -> (images (H,W,3) list, masks, backgrounds (N,3,H,W), records)"""
    rs = np.random.RandomState(77)
    cases = {}
    # blur clamping on both sides at once; SMOOTH's identity (H < 3 or W < 3) and its copied border
    for H, W in ((1, 1), (2, 3), (3, 3), (5, 7)):
        recs = [R(1, **ALL), R(2, **ALL), R(3, sharpness=50.0), R(0, bg=0, gate=0), R(2, bg=1, gray=1, color=0.4)]
        cases[f'tiny_{H}x{W}'] = ([make_frame(rs, H, W, 'random') for _ in recs], [make_mask(rs, H, W, 'mixed') for _ in recs],
                                  np.stack([make_frame(rs, H, W, 'random').transpose(2, 0, 1) for _ in range(2)]), recs)
    # factors at both ends of every interval, 0.0 and 1.0, one stage at a time; odd frame, not a multiple of anything
    recs = [R(1 + i % 3, **{name: f}) for i, (name, f) in enumerate(
        [('sharpness', 0.0), ('sharpness', 50.0), ('sharpness', 1.0), ('contrast', 0.2), ('contrast', 50.0), ('contrast', 0.0),
         ('contrast', 1.0), ('brightness', 0.1), ('brightness', 6.0), ('brightness', 0.0), ('brightness', 1.0), ('color', 0.0),
         ('color', 20.0), ('color', 1.0)])]
    H, W = 37, 53
    cases['factors_37x53'] = ([make_frame(rs, H, W, 'random' if i % 2 else 'mixed') for i in range(len(recs))], [make_mask(rs, H, W, 'full') for _ in recs],
                              np.zeros((0, 3, H, W), np.uint8), recs)
    # a batch whose images take every branch side by side: gate off, every k, stages present and absent, masks all zero / all non-zero /
    # mixed, constant 0 and constant 255 frames at factor 50 (both clip branches of blend and of SMOOTH)
    H, W = 48, 64
    recs = [R(1, **ALL, gray=1), R(gate=0, k=0), R(2, bg=0, sharpness=50.0, contrast=50.0), R(3, bg=1, contrast=50.0, sharpness=50.0, brightness=6.0, color=20.0),
            R(gate=0, k=0, bg=1), R(3, bg=0, brightness=0.1, gray=1), R(2, bg=1, color=0.0, contrast=0.2), R(0, bg=0, gate=0), R(3, sharpness=0.0)]
    ims = [make_frame(rs, H, W) for _ in recs]
    ims[2][:], ims[3][:] = 0, 255
    masks = [make_mask(rs, H, W, kind) for kind in ('mixed', 'mixed', 'full', 'full', 'zero', 'mixed', 'zero', 'mixed', 'mixed')]
    cases['mixed_48x64'] = (ims, masks, np.stack([make_frame(rs, H, W).transpose(2, 0, 1) for _ in range(2)]), recs)
    # mean(L) of the image Contrast sees is exactly x.5: int(mean + 0.5) must round it up
    H, W = 5, 6
    for _ in range(20000):
        im = make_frame(rs, H, W, 'random')
        blurred = np.asarray(PIL.Image.fromarray(im).filter(PIL.ImageFilter.GaussianBlur(1)).convert('L'))
        if 2 * int(blurred.sum()) % (2 * H * W) == H * W:
            break
    else:
        raise AssertionError('no frame with a half-integer mean found')
    cases['halfmean_5x6'] = ([im], [make_mask(rs, H, W, 'full')], np.zeros((0, 3, H, W), np.uint8), [R(1, contrast=1.7)])
    # more than one tile in both directions, by a non-multiple, in both tiled launches
    H, W = BIG_HW
    recs = [R(3, bg=0, **ALL), R(2, sharpness=21.0, contrast=0.6, gray=1)]
    cases[f'big_{H}x{W}'] = ([make_frame(rs, H, W) for _ in recs], [make_mask(rs, H, W, 'mixed') for _ in recs],
                             make_frame(rs, H, W)[None].transpose(0, 3, 1, 2), recs)
    return cases


def record_case(arrays, name, ims, masks, backgrounds, results):
    B = len(ims)
    arrays[f'{name}_images'] = np.stack([im.transpose(2, 0, 1) for im in ims])
    arrays[f'{name}_masks'] = np.stack(masks)
    arrays[f'{name}_backgrounds'] = backgrounds
    arrays[f'{name}_out'] = np.stack([res[0].transpose(2, 0, 1) for res in results])
    arrays[f'{name}_rec'] = np.array([[float(res[1][f]) for f in REC_FIELDS] for res in results], np.float64).reshape(B, len(REC_FIELDS))
    for st in STAGE_NAMES:
        idx = [b for b in range(B) if st in results[b][2]]
        if idx:
            arrays[f'{name}_stage_{st}_idx'] = np.array(idx, np.int32)
            arrays[f'{name}_stage_{st}'] = np.stack([results[b][2][st].transpose(2, 0, 1) for b in idx])


def main():
    A, rec = reference()
    torch.set_num_threads(1)
    arrays = {'pil_version': np.array(PIL.__version__), 'seeds': np.array(SEEDS, np.int32), 'rec_fields': np.array(REC_FIELDS),
              'stage_names': np.array(STAGE_NAMES)}
    covered = set()
    for s in SEEDS:
        rs = np.random.RandomState(1000 + s)
        H, W = SEEDED_HW
        ims = [make_frame(rs, H, W) for _ in range(N_SEEDED)]
        masks = [make_mask(rs, H, W, 'mixed') for _ in range(N_SEEDED)]
        backgrounds = np.stack([make_frame(rs, H, W).transpose(2, 0, 1) for _ in range(N_BG)])
        random.seed(s)
        rec.script = None
        results, draws = [], np.full((N_SEEDED, MAX_DRAWS, 2), np.nan)
        for b in range(N_SEEDED):
            rec.log = []
            results.append(chain(A, rec, ims[b], masks[b], backgrounds, True, True, True))
            for j, (kind, v) in enumerate(rec.log):
                draws[b, j] = KIND[kind], v
            r = results[-1][1]
            covered |= {('gate', r['gate']), ('bg', r['bg'] >= 0)}
            if r['gate']:
                covered |= {('k', r['k']), ('gray', r['gray'])} | {(n, not np.isnan(r[n])) for n in STAGE_NAMES[2:6]}
        arrays[f'seed{s}_draws'] = draws
        arrays[f'seed{s}_next'] = np.array(random.random())
        record_case(arrays, f'seed{s}', ims, masks, backgrounds, results)
    want = {('gate', 0), ('gate', 1), ('bg', True), ('bg', False), ('k', 1), ('k', 2), ('k', 3), ('gray', 0), ('gray', 1)} | \
        {(n, t) for n in STAGE_NAMES[2:6] for t in (True, False)}
    assert covered == want, want - covered

    forced = forced_cases(A, rec)
    for name, (ims, masks, backgrounds, recs) in forced.items():
        results = []
        for im, mask, r in zip(ims, masks, recs):
            with_bg, with_gray = len(backgrounds) > 0, True
            rec.log, rec.script = [], script_for(r, with_bg, with_gray)
            results.append(chain(A, rec, im, mask, backgrounds, with_bg, True, with_gray))
            assert rec.script == [], (name, rec.script)
            got = results[-1][1]
            for f in REC_FIELDS:                                    # the classes did what the case asked for
                w = r.get(f)
                assert (np.isnan(got[f]) if w is None else got[f] == w), (name, f, got[f], w)
        record_case(arrays, name, ims, masks, backgrounds, results)
    arrays['forced_cases'] = np.array(list(forced))
    save_npz(OUT, arrays)
    print('wrote', OUT, OUT.stat().st_size, 'bytes; Pillow', PIL.__version__)


if __name__ == '__main__':
    main()

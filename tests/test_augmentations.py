"""Training augmentations on the GPU (cosypose_amd.augmentations.augment_batch, csrc/kernels_aug.hip).

Yardsticks, both exact -- every comparison is np.array_equal on uint8, there is no tolerance anywhere in this file:
1. tests/golden/reference_golden_aug.npz: what the reference's own classes gave under Pillow (generate_golden_aug.py), every case;
2. tests/aug_ref.py, the numpy twin that test_augmentations_host.py holds against every recorded stage, on further seeded batches.
Sizes: 1x1 .. 5x7 (clamping from both sides at once, SMOOTH's identity and border rules), 37x53 (odd everything: the byte-wise pointwise
kernel), 48x64 (the 4-pixel pointwise kernel), 67x131 and 130x259 (more than one 8x128 row tile and 64x64 column tile in both directions,
by a non-multiple).  Each test prints its mismatch counts before it asserts."""
import random
import types

import numpy as np
import pytest
import torch

import aug_ref
from conftest import REPO

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (2, 3), (3, 3), (5, 7), (37, 53), (48, 64), (67, 131), (130, 259))


@pytest.fixture(scope='module')
def golden_aug():
    return aug_ref.golden_cases(REPO / 'tests' / 'golden' / 'reference_golden_aug.npz')[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(images, recs, masks=None, backgrounds=None, **kw):
    from cosypose_amd.augmentations import augment_batch
    with_bg = backgrounds is not None and len(backgrounds) > 0
    out = augment_batch(dev(images), recs, masks=dev(masks) if with_bg else None, backgrounds=dev(backgrounds) if with_bg else None, **kw)
    return out.cpu().numpy()


def seeded_batch(seed, H, W, B=5, n_bg=2):
    """B frames with records drawn as a dataset would draw them; the first three records are then forced onto the branches a small
    draw may miss (gate off with a paste, everything on, nothing but the blur)"""
    from cosypose_amd.augmentations import draw_sample_params
    rs, rng = np.random.RandomState(seed), random.Random(seed)
    images = rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    images[1] = (np.add.outer(np.arange(H) * 3, np.arange(W) * 5) % 256).astype(np.uint8)
    masks = (rs.rand(B, H, W) < 0.5).astype(np.uint8) * 3
    backgrounds = rs.randint(0, 256, (n_bg, 3, H, W)).astype(np.uint8)
    recs = [draw_sample_params(rng, gray_augmentation=True, n_backgrounds=n_bg) for _ in range(B)]
    recs[0] = dict(recs[0], gate=False, k=0, bg=1, sharpness=None, contrast=None, brightness=None, color=None, gray=False)
    recs[1] = dict(bg=0, gate=True, k=1 + seed % 3, sharpness=rng.uniform(0, 50), contrast=rng.uniform(0.2, 50), brightness=rng.uniform(0.1, 6),
                   color=rng.uniform(0, 20), gray=bool(seed % 2))
    recs[2] = dict(bg=-1, gate=True, k=1 + (seed + 1) % 3, sharpness=None, contrast=None, brightness=None, color=None, gray=False)
    return images, masks, backgrounds, recs


def test_every_fixture_case_byte_for_byte(golden_aug):
    bad = {}
    for name, c in golden_aug.items():
        got = run(c['images'], c['recs'], c['masks'], c['backgrounds'])
        bad[name] = int((got != c['out']).sum())
        print(f'{name}: {bad[name]} of {got.size} bytes differ from Pillow')
    assert len(bad) >= 12 and not any(bad.values()), bad
    for name, c in golden_aug.items():
        assert np.array_equal(run(c['images'], c['recs'], c['masks'], c['backgrounds']), c['out']), name


@pytest.mark.parametrize('hw', SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_seeded_batches_equal_the_twin(hw):
    for seed in (11, 12, 13):
        images, masks, backgrounds, recs = seeded_batch(seed, *hw)
        want = aug_ref.augment(images, recs, masks, backgrounds)
        got = run(images, recs, masks, backgrounds)
        print(f'{hw} seed {seed}: {int((got != want).sum())} of {got.size} bytes differ; per image {[(g != w).sum() for g, w in zip(got, want)]}')
        assert np.array_equal(got, want)
        assert np.array_equal(run(images, recs, masks, backgrounds), got)                  # a second run gives the same bytes


@pytest.mark.parametrize('hw', ((37, 53), (67, 131)), ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_an_image_alone_and_in_any_position(hw):
    images, masks, backgrounds, recs = seeded_batch(21, *hw)
    whole = run(images, recs, masks, backgrounds)
    for b in range(len(recs)):
        alone = run(images[b:b + 1], recs[b:b + 1], masks[b:b + 1], backgrounds)
        assert np.array_equal(alone[0], whole[b]), b
    order = [3, 0, 4, 2, 1]
    moved = run(images[order], [recs[i] for i in order], masks[order], backgrounds)
    assert np.array_equal(moved, whole[order])


@pytest.mark.parametrize('hw', ((37, 53), (48, 64)), ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_out_may_be_the_input_or_any_byte_address(hw):
    """`images` is read by the first launch only and `out` written by the last (and, point by point, by the images whose gate is off), so
    out = images is supported; an `out` that is not 4-byte aligned takes the byte-wise pointwise kernel."""
    from cosypose_amd.augmentations import augment_batch, pack_params
    images, masks, backgrounds, recs = seeded_batch(31, *hw)
    want = run(images, recs, masks, backgrounds)
    x = dev(images)
    y = augment_batch(x, recs, masks=dev(masks), backgrounds=dev(backgrounds), out=x)
    assert y is x and np.array_equal(x.cpu().numpy(), want)
    odd = torch.zeros(images.size + 1, dtype=torch.uint8, device='cuda')[1:].view(images.shape)
    assert odd.data_ptr() % 4 == 1
    augment_batch(dev(images), recs, masks=dev(masks), backgrounds=dev(backgrounds), out=odd)
    assert np.array_equal(odd.cpu().numpy(), want)
    table = torch.from_numpy(pack_params(recs).view(np.int32).reshape(-1, 8)).cuda()      # the table may already be on the device
    assert np.array_equal(augment_batch(dev(images), table, masks=dev(masks), backgrounds=dev(backgrounds)).cpu().numpy(), want)


def test_refusals():
    from cosypose_amd import _lib
    from cosypose_amd.augmentations import augment_batch
    images, masks, backgrounds, recs = seeded_batch(41, 5, 7)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        augment_batch(torch.from_numpy(images), recs)
    with pytest.raises(ValueError, match='background'):
        augment_batch(dev(images), recs)                                   # records name backgrounds, none given
    with pytest.raises(ValueError, match='uint8'):
        augment_batch(dev(images).float(), recs, masks=dev(masks), backgrounds=dev(backgrounds))
    with pytest.raises(ValueError, match='records'):
        augment_batch(dev(images), recs[:2], masks=dev(masks), backgrounds=dev(backgrounds))
    with pytest.raises(ValueError, match='out'):
        augment_batch(dev(images), recs, masks=dev(masks), backgrounds=dev(backgrounds), out=torch.empty(1, 3, 5, 7, dtype=torch.uint8, device='cuda'))
    # a table that reaches the device unchecked: a background row or a radius outside its range leaves the image as it is
    table = torch.tensor([[7, 1, 2, 0, 0, 0, 0, 0], [-1, 1, 9, 0, 0, 0, 0, 0]], dtype=torch.int32, device='cuda')
    got = augment_batch(dev(images[:2]), table, masks=dev(masks[:2]), backgrounds=dev(backgrounds))
    assert np.array_equal(got.cpu().numpy(), images[:2])
    assert augment_batch(dev(images[:0]), []).shape == (0, 3, 5, 7)


def test_prefetcher_transform_hands_out_the_augmented_bytes():
    from cosypose_amd import training
    from cosypose_amd.augmentations import augment_batch
    H, W, n = 48, 64, 4
    batches, want_plain, want_aug = [], [], []
    bgs = None
    for j in range(n):
        images, masks, backgrounds, recs = seeded_batch(50 + j, H, W)
        bgs = backgrounds if bgs is None else bgs
        batches.append(types.SimpleNamespace(images=torch.from_numpy(images).pin_memory(), masks=torch.from_numpy(masks).pin_memory(),
                                             K=torch.full((5, 3, 3), float(j)), aug=recs))
        want_plain.append(images)
        want_aug.append(aug_ref.augment(images, recs, masks, bgs))
    bgs_d = dev(bgs)

    def transform(batch):
        batch.images = augment_batch(batch.images, batch.aug, masks=batch.masks, backgrounds=bgs_d, out=batch.images)
        return batch

    fields = training.DevicePrefetcher.FIELDS + ('masks',)
    busy = torch.randn(1024, 1024, device='cuda')
    got = []
    for b in training.DevicePrefetcher(batches, fields=fields, transform=transform):
        busy = busy * 1.0001                                              # queued work between the batches, no synchronisation
        got.append(b.images.clone())
    assert len(got) == n and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want_aug))
    # the same bytes as augment_batch called by hand on what the prefetcher uploads, and the uploads themselves are what they are today
    plain = [(b.images.clone(), b.masks.clone(), b.K.clone()) for b in training.DevicePrefetcher(batches, fields=fields)]
    assert all(np.array_equal(p[0].cpu().numpy(), w) for p, w in zip(plain, want_plain))
    assert all(torch.equal(p[2].cpu(), b.K) for p, b in zip(plain, batches))
    by_hand = [augment_batch(p[0], b.aug, masks=p[1], backgrounds=bgs_d) for p, b in zip(plain, batches)]
    assert all(torch.equal(h, g) for h, g in zip(by_hand, got))
    assert not batches[0].images.is_cuda and training.DevicePrefetcher(batches).transform is None

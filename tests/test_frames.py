"""The frames' own resize on the GPU (cosypose_amd.frames.resize_frames, csrc/kernels_frames.hip).

Yardsticks:
1. tests/frames_ref.py, the numpy restatement of section 18 that test_frames_host.py holds against torch's generic kernel float for float:
   the device equals it ON EVERY BYTE (np.array_equal, no tolerance), flat and dyadic content included -- images, masks, K, boxes.
2. tests/golden/reference_golden_frames.npz, what the reference's CropResizeToAspectAugmentation gave: under section 18's parity rule (no
   byte differs outside the bytes whose exact value lies within 1e-4 of an integer, at most 1 % of a case; one level at most inside; masks,
   boxes and crop_resize_bbox equal; K within 2e-6 relative), the rule test_frames_host.py holds the restatement to.
Shapes: 3x4 and 1x1 sources (every tap clamped), 2:1, 4:1 and 5:1 downscales (dyadic weights; taps that skip rows), up- and downscales by
odd ratios, outputs of more than one 8-row x 128-byte tile in both directions, an output width of 30 (no dword stores, a partial last
thread), a square target, lists of mixed sizes with a frame already at size.  Each test prints its mismatch counts before it asserts."""
import unittest.mock

import numpy as np
import pytest
import torch

import frames_ref
from conftest import REPO, rel_err

pytestmark = pytest.mark.gpu

MAX_NEAR_SHARE = 0.01
K_TOL = 2e-6


@pytest.fixture(scope='module')
def golden_frames():
    g = np.load(REPO / 'tests' / 'golden' / 'reference_golden_frames.npz')
    return {str(name): {key: g[f'{name}_{key}'] for key in ('image', 'mask', 'K', 'resize', 'out_image', 'out_mask', 'out_K', 'bbox', 'boxes', 'resized')}
            for name in g['cases']}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_frame(rs, h, w, content='random'):
    if content == 'flat':                        # regions of 255 / 77 / 0: every byte inside one is an exact integer
        im = np.zeros((3, h, w), np.uint8)
        im[:, :h // 2, :w // 2], im[:, h // 3:, w // 2:] = 255, 77
        im[1, h // 2:, :w // 3] = 255
        return im
    return rs.randint(0, 256, (3, h, w)).astype(np.uint8)


def make_mask(rs, h, w):
    m = np.zeros((h, w), np.uint8)
    for i in (1, 2, 3, 5):
        hh, ww = rs.randint(1, max(h // 2, 1) + 1), rs.randint(1, max(w // 2, 1) + 1)
        y0, x0 = rs.randint(0, h - hh + 1), rs.randint(0, w - ww + 1)
        m[y0:y0 + hh, x0:x0 + ww] = i
    m[rs.rand(h, w) < 0.05] = 200
    return m


def make_K(rs, w, h):
    return np.array([[rs.uniform(0.8, 1.6) * w, 0, w / 2 + rs.uniform(-5, 5)], [0, rs.uniform(0.8, 1.6) * w, h / 2 + rs.uniform(-5, 5)], [0, 0, 1]])


def want_frames(images, resize, masks=None, K=None):
    per = [frames_ref.resize_frame(im, resize, None if masks is None else masks[i], None if K is None else K[i]) for i, im in enumerate(images)]
    return dict(images=np.stack([p['image'] for p in per]), masks=None if masks is None else np.stack([p['mask'] for p in per]),
                K=None if K is None else np.stack([p['K'] for p in per]), bbox=np.array([p['crop_resize_bbox'] for p in per], np.float64))


def check(got, want, label):
    bad = int((got.images.cpu().numpy() != want['images']).sum())
    bad_m = 0 if want['masks'] is None else int((got.masks.cpu().numpy() != want['masks']).sum())
    print(f'{label}: {bad} of {want["images"].size} image bytes and {bad_m} mask bytes differ from the definition')
    assert got.images.dtype == torch.uint8 and got.images.is_cuda and tuple(got.images.shape) == want['images'].shape
    assert np.array_equal(got.images.cpu().numpy(), want['images'])
    if want['masks'] is None:
        assert got.masks is None and got.stats is None
    else:
        assert got.masks.dtype == torch.uint8 and np.array_equal(got.masks.cpu().numpy(), want['masks'])
    if want['K'] is None:
        assert got.K is None
    else:
        assert got.K.dtype == torch.float32 and np.array_equal(got.K.cpu().numpy(), want['K'])
    assert isinstance(got.crop_resize_bbox, np.ndarray) and np.array_equal(got.crop_resize_bbox, want['bbox'])


# h, w, resize argument, content
SHAPES = ((3, 4, (16, 12), 'random'), (1, 1, (3, 3), 'random'), (96, 128, (64, 48), 'random'), (96, 128, (64, 48), 'flat'), (12, 16, (64, 48), 'random'),
          (54, 72, (64, 48), 'flat'), (99, 132, (64, 48), 'random'), (150, 200, (128, 96), 'random'), (150, 200, (96, 128), 'flat'),
          (50, 50, (32, 32), 'random'), (240, 320, (64, 48), 'random'), (33, 45, (30, 22), 'random'), (33, 45, (22, 30), 'flat'))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}_to_{min(s[2])}x{max(s[2])}_{s[3]}')
def test_every_byte_equals_the_definition(shape):
    from cosypose_amd import resize_frames
    h, w, resize, content = shape
    rs = np.random.RandomState(h * 1000 + w)
    images = [make_frame(rs, h, w, content), make_frame(rs, h, w)]
    masks = [make_mask(rs, h, w) for _ in images]
    K = np.stack([make_K(rs, w, h) for _ in images])
    want = want_frames(images, resize, masks, K)
    got = resize_frames([dev(im) for im in images], resize, masks=[dev(m) for m in masks], K=K)
    check(got, want, str(shape))
    again = resize_frames([dev(im) for im in images], resize, masks=[dev(m) for m in masks], K=K)
    assert torch.equal(again.images, got.images) and torch.equal(again.masks, got.masks) and torch.equal(again.K, got.K)   # the same bits


def test_one_pixel_source_to_3x4():
    """1x1 -> 3x4: the aspect test refuses it (1 is not 4/3), so it is lifted for this call; every tap of both axes is clamped to the one
    pixel, and the byte is what the definition makes of it"""
    from cosypose_amd import frames
    image = np.array([[[201]], [[7]], [[255]]], np.uint8)
    mask = np.array([[9]], np.uint8)
    with pytest.raises(ValueError, match='aspect'):
        frames.resize_frames([dev(image)], (4, 3))
    with unittest.mock.patch.object(frames, 'check_aspect', lambda *a: None):
        got = frames.resize_frames([dev(image)], (4, 3), masks=[dev(mask)])
    want = frames_ref.image_bytes(image, 3, 4)
    print('1x1 -> 3x4:', got.images.cpu().numpy().reshape(3, -1).tolist(), want.reshape(3, -1).tolist())
    assert np.array_equal(got.images[0].cpu().numpy(), want) and (got.masks.cpu().numpy() == 9).all() and tuple(got.masks.shape) == (1, 3, 4)


@pytest.fixture(scope='module')
def mixed():
    """five sizes and a frame already at 48x64, masks and K with them, and the definition's results"""
    rs = np.random.RandomState(1848)
    sizes = ((99, 132), (45, 60), (48, 64), (54, 72), (150, 200), (240, 320))
    images = [make_frame(rs, h, w, 'flat' if i == 3 else 'random') for i, (h, w) in enumerate(sizes)]
    masks = [make_mask(rs, h, w) for h, w in sizes]
    K = np.stack([make_K(rs, w, h) for h, w in sizes])
    return images, masks, K, want_frames(images, (64, 48), masks, K)


def test_one_list_of_mixed_sizes_with_an_identity_frame(mixed):
    from cosypose_amd import resize_frames
    images, masks, K, want = mixed
    got = resize_frames([dev(im) for im in images], (64, 48), masks=[dev(m) for m in masks], K=dev(K))
    check(got, want, 'mixed list')
    assert got.K.is_cuda                                                        # K comes back on the side it came from
    assert np.array_equal(got.images[2].cpu().numpy(), images[2]) and np.array_equal(got.masks[2].cpu().numpy(), masks[2])
    assert np.array_equal(got.K[2].cpu().numpy(), K[2].astype(np.float32))
    assert got.crop_resize_bbox[2].tolist() == [0, 0, 63, 47] and got.crop_resize_bbox[0].tolist() == [0, 0, 132, 99]


def test_batch_tensor_input_and_given_outputs(mixed):
    from cosypose_amd import resize_frames
    rs = np.random.RandomState(7)
    images = np.stack([make_frame(rs, 54, 72), make_frame(rs, 54, 72, 'flat'), make_frame(rs, 54, 72)])
    masks = np.stack([make_mask(rs, 54, 72) for _ in images])
    want = want_frames(images, (64, 48), masks)
    out = torch.full((3, 3, 48, 64), 99, dtype=torch.uint8, device='cuda')
    out_masks = torch.full((3, 48, 64), 99, dtype=torch.uint8, device='cuda')
    got = resize_frames(dev(images), (64, 48), masks=dev(masks), out=out, out_masks=out_masks)
    assert got.images is out and got.masks is out_masks and got.K is None and got.stats is None
    check(got, want, '(N,3,h,w) tensor, out= and out_masks=')
    # a batch already at size: copied, and the bbox is the reference's (0, 0, w - 1, h - 1)
    same = resize_frames(dev(want['images']), (64, 48), masks=dev(want['masks']))
    assert torch.equal(same.images, got.images) and torch.equal(same.masks, got.masks) and same.crop_resize_bbox.tolist() == [[0, 0, 63, 47]] * 3


def test_masks_absent(mixed):
    from cosypose_amd import resize_frames
    images, _, K, want = mixed
    got = resize_frames([dev(im) for im in images], (64, 48), K=torch.from_numpy(K))
    check(got, dict(want, masks=None), 'no masks')
    assert not got.K.is_cuda


def test_boxes_are_the_stats_of_the_resized_masks(mixed, golden_frames):
    from cosypose_amd import resize_frames
    from cosypose_amd.mask_ops import mask_instance_stats
    images, masks, K, want = mixed
    got = resize_frames([dev(im) for im in images], (64, 48), masks=[dev(m) for m in masks], boxes=True)
    assert got.stats.dtype == torch.int32 and tuple(got.stats.shape) == (len(images), 256, 5)
    assert torch.equal(got.stats, mask_instance_stats(got.masks))
    for i, m in enumerate(want['masks']):
        assert np.array_equal(got.stats[i, :6].cpu().numpy(), frames_ref.instance_stats(m, 6)), i
    # the fixture's refreshed boxes, case by case (each case has a target of its own)
    for name, c in golden_frames.items():
        if not c['resized']:
            continue
        got = resize_frames([dev(c['image'])], tuple(c['resize']), masks=[dev(c['mask'])], boxes=True)
        boxes = got.stats[0, :6, 1:].cpu().numpy()
        print(name, boxes.tolist())
        assert np.array_equal(boxes, c['boxes']), name


def test_fixture_cases_under_the_parity_rule(golden_frames):
    from cosypose_amd import resize_frames
    assert len(golden_frames) == 6
    for name, c in golden_frames.items():
        got = resize_frames([dev(c['image'])], tuple(c['resize']), masks=[dev(c['mask'])], K=c['K'][None])
        image, H, W = got.images[0].cpu().numpy(), *got.images.shape[2:]
        if c['resized']:
            outside, inside, share = frames_ref.parity_report(image, c['out_image'], frames_ref.image_exact(c['image'], H, W))
            print(f'{name}: {outside} bytes differ outside the near-integer set, largest difference inside {inside}, share {100 * share:.3f} %')
            assert outside == 0 and inside <= 1 and share <= MAX_NEAR_SHARE, name
        else:
            assert np.array_equal(image, c['out_image']), name
        assert np.array_equal(got.masks[0].cpu().numpy(), c['out_mask']), name
        assert tuple(got.crop_resize_bbox[0]) == tuple(c['bbox']), name
        assert rel_err(got.K[0].numpy(), c['out_K']) < K_TOL, name


def test_wrong_aspect_and_cpu_tensors_raise_before_any_launch(mixed):
    from cosypose_amd import _lib, resize_frames
    images = mixed[0]
    out = torch.full((2, 3, 48, 64), 123, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match=r'frame 1 is 52x64.*1\.23077.*1\.33333'):
        resize_frames([dev(images[0]), dev(np.zeros((3, 52, 64), np.uint8))], (64, 48), out=out)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_frames([dev(images[0]), torch.from_numpy(images[1])], (64, 48), out=out)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_frames([dev(images[0]), dev(images[1])], (64, 48), masks=[torch.zeros(99, 132, dtype=torch.uint8), torch.zeros(45, 60, dtype=torch.uint8)], out=out)
    torch.cuda.synchronize()
    assert (out == 123).all()

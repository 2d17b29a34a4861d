"""Image resize on the GPU (cosypose_amd.resize.resize_images, csrc/kernels_resize.hip).

Yardsticks, both exact -- every comparison is np.array_equal on uint8, there is no tolerance anywhere in this file:
1. tests/golden/pillow_resize.npz: what Pillow 12.2.0's Image.resize gave with BILINEAR and BICUBIC (generate_golden_resize.py), every case;
2. tests/resize_ref.py, the numpy twin that test_resize_host.py holds against those bytes and against live Pillow, on further seeded batches.
Sizes: 1x1 .. 5x7 (every tap clamped, one pass only), 24x32 (copy), 37x53 -> 48x64 (the VOC-like ratio, odd rows: the byte-wise loads and
stores), 97x211 -> 24x32 (29 taps), 131x67 -> 70x150 and the seeded ones up to 130x260 -> 150x300 (more than one 4-row x 256-byte tile in
both directions, by a non-multiple), 300x8 -> 6x8 (201 taps).  Pillow is not needed here.  Each test prints its mismatch counts before it
asserts."""
import random

import numpy as np
import pytest
import torch

import aug_ref
import resize_ref
from conftest import REPO

pytestmark = pytest.mark.gpu

FILTERS = ('bilinear', 'bicubic')
MIXED = ('2x3_to_5x7', '5x7_to_5x9', '37x53_to_48x64', '97x211_to_24x32', '131x67_to_70x150', '300x8_to_6x8', '24x32_to_24x32')


@pytest.fixture(scope='module')
def golden_resize():
    return resize_ref.golden_cases(REPO / 'tests' / 'golden' / 'pillow_resize.npz')[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(images, size, resample='bicubic', **kw):
    from cosypose_amd.resize import resize_images
    images = dev(images) if isinstance(images, np.ndarray) else [dev(im) for im in images]
    return resize_images(images, size, resample, **kw).cpu().numpy()


def mixed_list(golden_resize, size):
    """images of seven different sizes from the fixture, two contents each, with the per-image twin results at `size`"""
    images = [golden_resize[name]['images'][j] for name in MIXED for j in (0, 3)]
    return images, {f: np.stack([resize_ref.resize(im, size, f) for im in images]) for f in FILTERS}


def test_every_fixture_case_byte_for_byte(golden_resize):
    bad = {}
    for name, c in golden_resize.items():
        for f in FILTERS:
            got = run(c['images'], c['size'], f)
            bad[name, f] = int((got != c[f]).sum())
            print(f'{name} {f}: {bad[name, f]} of {got.size} bytes differ from Pillow')
    assert len(bad) == 24 and not any(bad.values()), bad


@pytest.mark.parametrize('shape', ((1, 1, 3, 2), (7, 5, 7, 11), (33, 67, 48, 64), (130, 260, 150, 300), (129, 259, 40, 300), (64, 300, 64, 257)),
                         ids=lambda s: f'{s[0]}x{s[1]}_to_{s[2]}x{s[3]}')
def test_seeded_batches_equal_the_twin(shape):
    h, w, H, W = shape
    rs = np.random.RandomState(h * 1000 + w)
    for C in (3, 1):
        images = rs.randint(0, 256, (3, C, h, w)).astype(np.uint8)
        images[1] = (rs.randint(0, 2, (C, h, w)) * 255).astype(np.uint8)
        for f in FILTERS:
            want = resize_ref.resize_batch(images, (H, W), f)
            got = run(images, (H, W), f)
            print(f'{shape} C={C} {f}: {int((got != want).sum())} of {got.size} bytes differ')
            assert np.array_equal(got, want)
            assert np.array_equal(run(images, (H, W), f), got)                 # a second call gives the same bytes


def test_one_call_on_a_list_of_mixed_sizes(golden_resize):
    from cosypose_amd import _lib
    from cosypose_amd.resize import resize_images
    size = (48, 64)
    images, want = mixed_list(golden_resize, size)
    assert len({im.shape for im in images}) >= 4
    lib = _lib.lib()
    calls = []
    real = lib.cosy_resize_u8

    def counted(*args):
        calls.append(args[1])
        return real(*args)

    for f in FILTERS:
        lib.cosy_resize_u8 = counted
        try:
            got = resize_images([dev(im) for im in images], size, f).cpu().numpy()
        finally:
            lib.cosy_resize_u8 = real
        print(f'{f}: {int((got != want[f]).sum())} of {got.size} bytes differ; per image {[int((g != w).sum()) for g, w in zip(got, want[f])]}')
        assert np.array_equal(got, want[f])
    assert calls == [len(images)] * 2                                           # the whole list went through ONE call of the library, each time


def test_an_image_alone_and_in_any_position(golden_resize):
    size = (70, 150)
    images, want = mixed_list(golden_resize, size)
    whole = run(images, size)
    assert np.array_equal(whole, want['bicubic'])
    for b in (0, 5, 9, len(images) - 1):
        assert np.array_equal(run([images[b]], size)[0], whole[b]), b
    order = list(range(len(images)))
    random.Random(3).shuffle(order)
    assert np.array_equal(run([images[i] for i in order], size), whole[order])


@pytest.mark.parametrize('size', ((48, 64), (37, 53), (35, 51)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_out_at_any_byte_address(golden_resize, size):
    """(48, 64): rows that are 4-byte aligned in a fresh `out`; (37, 53) holds images already at size (a copy) and odd rows; an `out` at
    an odd byte offset into a larger buffer takes the byte-wise stores everywhere"""
    from cosypose_amd.resize import resize_images
    images = [golden_resize[name]['images'][0] for name in ('37x53_to_48x64', '131x67_to_70x150', '5x7_to_8x7')]
    want = resize_ref.resize_batch(images, size)
    out = torch.full((3, 3) + size, 7, dtype=torch.uint8, device='cuda')
    got = resize_images([dev(im) for im in images], size, out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want)
    for offset in (1, 2, 3):
        buf = torch.full((want.size + 8,), 9, dtype=torch.uint8, device='cuda')
        odd = buf[offset:offset + want.size].view(want.shape)
        assert odd.data_ptr() % 4 == (buf.data_ptr() + offset) % 4 and odd.is_contiguous()
        resize_images([dev(im) for im in images], size, out=odd)
        host = buf.cpu().numpy()
        assert np.array_equal(host[offset:offset + want.size].reshape(want.shape), want), offset
        assert (host[:offset] == 9).all() and (host[offset + want.size:] == 9).all(), offset        # nothing written around it
    with pytest.raises(ValueError, match='out must be'):
        resize_images([dev(im) for im in images], size, out=torch.empty((3, 3) + size, dtype=torch.uint8, device='cuda').transpose(2, 3))
    with pytest.raises(ValueError, match='out must be'):
        resize_images([dev(im) for im in images], size, out=torch.empty((2, 3) + size, dtype=torch.uint8, device='cuda'))


def test_tensor_form_equals_list_form_and_the_empty_batch(golden_resize):
    from cosypose_amd.resize import resize_images
    c = golden_resize['131x67_to_70x150']
    for f in FILTERS:
        as_tensor = run(c['images'], c['size'], f)
        as_list = run(list(c['images']), c['size'], f)
        assert np.array_equal(as_tensor, as_list) and np.array_equal(as_tensor, c[f])
    sliced = dev(np.concatenate([c['images'], c['images']], axis=3))[:, :, :, :67]                 # not contiguous: made so, same bytes
    assert not sliced.is_contiguous() and np.array_equal(resize_images(sliced, c['size']).cpu().numpy(), c['bicubic'])
    for C in (1, 3):
        empty = resize_images(torch.empty(0, C, 9, 11, dtype=torch.uint8, device='cuda'), (4, 6))
        assert empty.shape == (0, C, 4, 6) and empty.dtype == torch.uint8 and empty.is_cuda
    out = torch.empty(0, 3, 4, 6, dtype=torch.uint8, device='cuda')
    assert resize_images([], (4, 6), out=out) is out
    with pytest.raises(ValueError, match='empty list'):
        resize_images([], (4, 6))


def test_a_descriptor_the_kernel_cannot_serve_leaves_its_output_untouched():
    """the public function never builds such a table; this one goes to the library by hand: a table offset outside the tables, a source
    taller than max_h, a skipped pass whose lengths differ, and a bounds entry that would read past its line"""
    from cosypose_amd import _lib, resize
    H, W, h, w = 6, 9, 5, 7
    rs = np.random.RandomState(1)
    src = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
    src_d = dev(src)
    hb, hk = resize.axis_tables(w, W, 'bicubic')
    vb, vk = resize.axis_tables(h, H, 'bicubic')
    bad_b = hb.copy()
    bad_b[4] = (w - 1, 3)                                                       # three taps from the last pixel on
    parts = [hb.reshape(-1), hk.reshape(-1), vb.reshape(-1), vk.reshape(-1), bad_b.reshape(-1)]
    offs = np.cumsum([0] + [p.size for p in parts])
    n_tables = int(offs[-1])
    good = dict(src=src_d.data_ptr(), h=h, w=w, hb=offs[0], hk=offs[1], hks=hk.shape[1], vb=offs[2], vk=offs[3], vks=vk.shape[1])
    rows = [good, dict(good, hk=n_tables - 3), dict(good, vb=-1), dict(good, h=h + 1), dict(good, hks=0, hb=0, hk=0), dict(good, src=0),
            dict(good, hb=offs[4]), good]
    items = np.zeros(len(rows), resize.ITEM_DTYPE)
    for row, r in zip(items, rows):
        for key, v in r.items():
            row[key] = v
    blob = np.concatenate([items.view(np.uint8), np.concatenate(parts).view(np.uint8)])
    blob_d = dev(blob)
    out = torch.full((len(rows), 3, H, W), 77, dtype=torch.uint8, device='cuda')
    lib = _lib.lib()
    ws_bytes = lib.cosy_resize_workspace_bytes(len(rows), 3, h, W)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    _lib.check(lib.cosy_resize_u8(blob_d.data_ptr(), len(rows), 3, H, W, h, blob_d.data_ptr() + items.nbytes, n_tables, out.data_ptr(),
                                  ws.data_ptr(), ws_bytes, _lib.stream()))
    got = out.cpu().numpy()
    want = resize_ref.resize(src, (H, W))
    assert np.array_equal(got[0], want) and np.array_equal(got[7], want)
    for i in (1, 2, 3, 4, 5):
        assert (got[i] == 77).all(), i
    # the row with one bad bounds entry: every column but that one is served; the bad one holds what the zeroed workspace gives
    cols = [x for x in range(W) if x != 4]
    assert np.array_equal(got[6][:, :, cols], want[:, :, cols])
    with pytest.raises(_lib.CosyHipError, match='workspace_bytes'):
        _lib.check(lib.cosy_resize_u8(blob_d.data_ptr(), len(rows), 3, H, W, h, blob_d.data_ptr() + items.nbytes, n_tables, out.data_ptr(),
                                      ws.data_ptr(), ws_bytes - 256, _lib.stream()))


def test_resized_backgrounds_feed_augment_batch(golden_resize):
    """resize_images -> augment_batch(backgrounds=...) reproduces the twin chain resize_ref -> aug_ref.augment"""
    from cosypose_amd.augmentations import augment_batch, draw_sample_params
    from cosypose_amd.resize import resize_images
    H, W, B = 48, 64, 6
    raw = [golden_resize[name]['images'][0] for name in ('37x53_to_48x64', '97x211_to_24x32', '131x67_to_70x150', '5x7_to_8x7')]
    rs, rng = np.random.RandomState(8), random.Random(8)
    raw.append(rs.randint(0, 256, (3, H, W)).astype(np.uint8))                  # one already at frame size
    images = rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    masks = (rs.rand(B, H, W) < 0.5).astype(np.uint8)
    recs = [draw_sample_params(rng, gray_augmentation=True, background_p=1.0, n_backgrounds=len(raw)) for _ in range(B)]
    recs[0] = dict(recs[0], bg=4)
    recs[1] = dict(recs[1], bg=2, gate=False, k=0, sharpness=None, contrast=None, brightness=None, color=None, gray=False)
    assert {r['bg'] for r in recs} >= {2, 4} and all(r['bg'] >= 0 for r in recs)
    backgrounds = resize_images([dev(im) for im in raw], (H, W))
    want_bg = resize_ref.resize_batch(raw, (H, W))
    assert np.array_equal(backgrounds.cpu().numpy(), want_bg)
    got = augment_batch(dev(images), recs, masks=dev(masks), backgrounds=backgrounds).cpu().numpy()
    want = aug_ref.augment(images, recs, masks, want_bg)
    print(f'{int((got != want).sum())} of {got.size} bytes differ')
    assert np.array_equal(got, want)

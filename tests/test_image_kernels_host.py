"""CPU side of test_image_kernels.py: every coverage condition that the GPU file relies on, proved on the numpy twins alone (aug_ref,
resize_ref, frames_ref) and on the very inputs that tests/image_edge_case.py hands to both files.  A GPU test that claims to reach the
ends of the byte range, an exact tie of Contrast's mean or the extremes of the bicubic accumulator is only as good as its inputs: here
the inputs are shown to do so, without any kernel.  No tolerance anywhere; each test prints its figures before it asserts."""
import numpy as np
import pytest

import aug_ref
import frames_ref
import image_edge_case as case
import resize_ref

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------- A1
@pytest.fixture(scope='module')
def blurred_values256():
    image, colours = case.values256()
    return {k: aug_ref.gaussian_blur(case.hwc(image), k) for k in (1, 2, 3)}


def test_block_centres_survive_the_blur_and_every_value_is_there(blurred_values256):
    image, colours = case.values256()
    assert image.shape == (3, 320, 320) and all(sorted(colours[:, c]) == list(range(256)) for c in range(3))
    for k, blurred in blurred_values256.items():
        centres = case.block_centres(blurred.transpose(2, 0, 1), 16)
        held = [len(np.unique(blurred[..., c])) for c in range(3)]
        print(f'values256 k={k}: {int((centres != colours).sum())} block centres changed; distinct values per channel {held}; '
              f'range {blurred.min()}..{blurred.max()}')
        assert np.array_equal(centres, colours)
        assert held == [256, 256, 256]
    big, big_colours = case.colours4096()
    assert big.shape == (3, 1280, 1280) and len({tuple(c) for c in big_colours}) == 4096 and set(np.unique(big_colours)) == set(range(0, 256, 17))
    blurred = aug_ref.gaussian_blur(case.hwc(big), 3)                              # the widest reach; k = 1 and 2 stay inside it
    assert np.array_equal(case.block_centres(blurred.transpose(2, 0, 1), 64), big_colours)


def test_single_stage_records_clip_at_the_ends_and_factor_one_is_the_identity(blurred_values256):
    image, _ = case.values256()
    records = dict(case.single_stage_records())
    assert len(records) == 21 and {r['k'] for r in records.values()} == {1, 2, 3}
    shares = {}
    for label in ('contrast=3.0', 'brightness=1.5', 'color=4.0'):
        r = records[label]
        im = blurred_values256[r['k']]
        deg = dict(contrast=lambda: np.full_like(im, aug_ref.contrast_mean(im)), brightness=lambda: np.zeros_like(im),
                   color=lambda: np.repeat(aug_ref.luma(im)[..., None], 3, axis=2))[label.split('=')[0]]()
        shares[label] = case.blend_clip_shares(deg, im, float(label.split('=')[1]))
        stages = []
        out = aug_ref.augment_one(case.hwc(image), r, stages=stages)
        assert [n for n, _ in stages] == ['blur', label.split('=')[0]] and np.array_equal(stages[0][1], im)
        ends = float((out == 0).mean()), float((out == 255).mean())
        print(f'{label} (k={r["k"]}): branch t <= 0 taken by {100 * shares[label][0]:.1f} %, t >= 255 by {100 * shares[label][1]:.1f} % of bytes; '
              f'output bytes at 0: {100 * ends[0]:.1f} %, at 255: {100 * ends[1]:.1f} %')
        assert ends[0] >= shares[label][0] - 1e-12 and ends[1] >= shares[label][1] - 1e-12
    assert min(shares['contrast=3.0']) >= 0.05 and min(shares['color=4.0']) >= 0.05
    assert shares['brightness=1.5'][1] >= 0.05 and shares['brightness=1.5'][0] < 0.01
    for label, r in records.items():
        if label.endswith('=1.0'):
            assert np.array_equal(aug_ref.augment_one(case.hwc(image), r), blurred_values256[r['k']]), label


def test_full_chain_on_colours4096_is_quick_on_the_twin():
    import time
    image, _ = case.colours4096()
    recs = case.full_chain_records()
    assert [r['k'] for r in recs] == [1, 2, 3] and [r['gray'] for r in recs] == [False, True, False]
    assert all(r[name] is not None for r in recs for name in aug_ref.STAGES)
    t0 = time.perf_counter()
    out = aug_ref.augment_one(case.hwc(image), recs[1])
    print(f'full twin chain on 1280x1280: {time.perf_counter() - t0:.2f} s; output range {out.min()}..{out.max()}')
    assert out.shape == (1280, 1280, 3)


@pytest.mark.parametrize('hw', ((3, 3), (20, 140)), ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_a_constant_frame_is_a_fixed_point_of_the_twin(hw):
    images, plain, sharp = case.constant_frames(*hw)
    changed = 0
    for v in range(256):
        for k in (1, 2, 3):                                                        # all 768 (value, k) cases
            changed += int((aug_ref.augment_one(case.hwc(images[v]), case.rec(k)) != v).sum())
    print(f'{hw}: {changed} bytes changed over 768 (value, k) cases')
    assert changed == 0
    assert [r['k'] for r in plain[:4]] == [1, 2, 3, 1] and all(r['sharpness'] == 2.0 for r in sharp)
    # SMOOTH of a constant goes through float32: whether 9 products of v / 13 and 5 v / 13 truncate back to v is the twin's to say
    out = aug_ref.augment(images, sharp)
    print(f'{hw} sharpness 2.0: {int((out != images).sum())} bytes of {out.size} leave their constant in the twin')


# ---------------------------------------------------------------- A2
def test_aug_edge_sizes_sit_on_the_tile_borders():
    rows = {(h % 8, w % 128) for h, w in case.AUG_EDGE_SIZES}
    cols = {(h % 64, w % 64) for h, w in case.AUG_EDGE_SIZES}
    assert {0, 1, 9, 10} <= {w for _, w in rows} | {h for h, _ in rows} and {0, 1, 10, 63} <= {h for h, _ in cols} and {0, 1, 2, 3, 63} <= {w for _, w in cols}
    for h, w in case.AUG_EDGE_SIZES:
        images, masks, backgrounds, recs = case.aug_edge_batch(h, w)
        assert images.shape == (8, 3, h, w) and masks.shape == (8, h, w) and backgrounds.shape == (2, 3, h, w)
        assert sum(r['bg'] >= 0 for r in recs) == 4 and {r['bg'] for r in recs} == {-1, 0, 1}
        assert sorted((r['k'], r['sharpness']) for r in recs[:4]) == [(1, None), (1, None), (3, 7.5), (3, 7.5)]
        assert set(np.unique(images[0])) == {0, 255} and 0.3 < (masks == 0).mean() < 0.7
        seam = images[2]
        assert np.array_equal(seam, images[3]) and set(np.unique(seam)) <= {0, 255}
        lit_x = [x for x in range(w) if (seam[0, :, x] == 255).all()]
        lit_y = [y for y in range(h) if (seam[0, y] == 255).all()]
        assert lit_x == [x for x in (127, 128) if x < w] and lit_y == [y for y in (7, 8, 63, 64) if y < h], (h, w)


# ---------------------------------------------------------------- A3
def test_contrast_mean_ties_are_real_and_the_mean_range_is_reached():
    ties = case.tie_frames()
    for image, mean in ties:
        s, n = case.blurred_l_sum(image)
        stages = []
        aug_ref.augment_one(case.hwc(image), case.rec(1, contrast=0.2), stages=stages)
        print(f'tie frame {image.shape[1]}x{image.shape[2]}: sum of L {s} over {n} pixels = {s / n}, mean {mean}')
        assert image.shape[1] <= 4 and image.shape[2] <= 4
        assert (2 * s + n) % (2 * n) == 0 and 2 * s == (2 * mean - 1) * n            # the mean of L is exactly mean - 1/2
        assert aug_ref.contrast_mean(stages[0][1]) == mean == int(s / n + 0.5)
    assert len(ties) >= 3 and len({m for _, m in ties}) == len(ties)
    frames = case.mean_range_frames()
    print('mean range frames:', {m: case.blurred_l_sum(f) for m, f in frames.items()})
    assert sorted(frames) == [0, 1, 254, 255]
    for mean, image in frames.items():
        s, n = case.blurred_l_sum(image)
        assert aug_ref.contrast_mean(aug_ref.gaussian_blur(case.hwc(image), 1)) == mean and 0 < s < 255 * n
    for h, w in case.HALF_SIZES:
        for vertical in (False, True):
            s, n = case.blurred_l_sum(case.half_frame(h, w, vertical))
            print(f'half frame {h}x{w} split along {"x" if vertical else "y"}: mean of L {s / n}')
            assert abs(s / n - 127.5) < 1.0


# ---------------------------------------------------------------- B1
@pytest.mark.parametrize('resample', case.FILTERS)
def test_resize_accumulators_fit_in_int32_and_reach_both_clips(resample):
    lo, hi = 0, 0
    for n_in, n_out in case.RESIZE_AXES:
        t = case.tap_sign_lines(n_in, n_out, resample)
        bounds, k = resize_ref.coeffs(n_in, n_out, resample)
        # every output index of every line of the image the GPU test runs, in Python integers
        image = case.tap_sign_image(n_in, n_out, resample)
        acc = np.array([[(1 << 21) + sum(int(p) * int(c) for p, c in zip(row[a:a + n], kk[:n])) for (a, n), kk in zip(bounds, k)]
                        for row in image[0]], dtype=object)
        assert acc[0, t['xx_pos']] == t['acc_pos'] == acc.max() and acc[1, t['xx_neg']] == t['acc_neg'] == acc.min()
        lo, hi = min(lo, t['acc_neg']), max(hi, t['acc_pos'])
        print(f'{resample} {n_in}->{n_out}: accumulator {t["acc_neg"]} (index {t["xx_neg"]}) .. {t["acc_pos"]} (index {t["xx_pos"]})')
        assert INT32_MIN <= t['acc_neg'] and t['acc_pos'] <= INT32_MAX
        for im, axis in ((image, 2), (np.ascontiguousarray(image.transpose(0, 2, 1)), 1)):
            size = (5, n_out) if axis == 2 else (n_out, 5)
            out = np.moveaxis(resize_ref.resize(im, size, resample), axis, 2)
            assert out[0, 0, t['xx_pos']] == 255 and out[0, 1, t['xx_neg']] == 0
        if k.min() < 0:                                                            # bicubic, but for 2000 -> 1 and 1 -> 9: one lobe only
            assert t['acc_neg'] < -(1 << 22) and t['acc_pos'] > 256 << 22, (n_in, n_out)  # below byte 0 and above byte 255 before the clip
    lobes = sum(resize_ref.coeffs(n_in, n_out, resample)[1].min() < 0 for n_in, n_out in case.RESIZE_AXES)
    assert lobes == (5 if resample == 'bicubic' else 0)
    print(f'{resample}: the accumulators span {lo} .. {hi}')
    assert hi <= 1_300_000_000 and lo >= -200_000_000                              # far inside int32: measured 1 206 351 992 and -132 610 168


# ---------------------------------------------------------------- B2
@pytest.mark.parametrize('resample', case.FILTERS)
def test_resize_twin_keeps_constants_constant(resample):
    for h, w, H, W in case.RESIZE_CONSTANT_SHAPES:
        images = case.constant_images(h, w)
        out = resize_ref.resize(images[:, 0], (H, W), resample)                    # the 256 images as 256 channels of one
        bad = int((out != np.arange(256, dtype=np.uint8)[:, None, None]).sum())
        print(f'{resample} {h}x{w} -> {H}x{W}: {bad} bytes of {out.size} leave their constant in the twin')
        assert bad == 0


# ---------------------------------------------------------------- B3
def test_resize_edge_shapes_cover_what_they_name():
    shapes = case.resize_edge_shapes()
    assert {(H, W) for _, _, H, W, _ in shapes} >= {(H, W) for H in case.RESIZE_EDGE_HEIGHTS for W in case.RESIZE_EDGE_WIDTHS}
    for W in case.RESIZE_EDGE_WIDTHS:
        assert {off for _, _, _, w_out, off in shapes[:32] if w_out == W} == {0, 1, 2, 3}
        assert len({(h, w) for h, w, _, w_out, _ in shapes[:32] if w_out == W}) == 2
    assert set(case.RESIZE_LONG_SHAPES) <= {s[:4] for s in shapes}
    assert resize_ref.coeffs(2000, 1, 'bicubic')[1].shape[1] == 8001
    images = case.resize_edge_images(6, 261, 3)
    assert images.shape == (2, 3, 6, 261) and set(np.unique(images[1])) == {0, 255}


# ---------------------------------------------------------------- C
def test_fma_emulation_accepts_every_frames_input():
    """frames_ref.fma32 raises DoubleRounding where it cannot promise one rounding: it must not, on any input of the GPU file"""
    n = 0
    for h, w, H, W in case.FRAME_CONSTANT_SHAPES:
        images, masks = case.frame_constants(h, w)
        out = frames_ref.image_bytes(images.reshape(-1, h, w), H, W)
        assert {int(v) for m in masks for v in np.unique(m)} == set(range(256))
        off = np.flatnonzero((out.reshape(256, -1) != np.arange(256)[:, None]).any(axis=1))
        print(f'constants {h}x{w} -> {H}x{W}: values that do not come back as themselves: {off.tolist()}')
        n += 1
    for h, w, H, W in case.FRAME_STRUCTURED_SHAPES:
        images, masks = case.frame_structured(h, w)
        out = frames_ref.image_bytes(images.reshape(-1, h, w), H, W)
        assert set(np.unique(images[0])) == {0, 255} and len(np.unique(images[1])) == 256 and len(np.unique(masks[0])) == 256
        print(f'structured {h}x{w} -> {H}x{W}: output range {out.min()}..{out.max()}')
        n += 1
    for (H, W), sources in case.FRAME_EDGE_SHAPES.items():
        (uh, uw), (dh, dw) = sources
        assert uh < H and dh > H and uw * H == uh * W and dw * H == dh * W
        for h, w in sources:
            images, masks = case.frame_edge_inputs(h, w)
            frames_ref.image_bytes(images.reshape(-1, h, w), H, W)
            n += 1
    assert n == 16
    assert {(H % 8, W % 128) for H, W in case.FRAME_EDGE_SHAPES} == {(5, 124), (0, 0), (3, 4)}

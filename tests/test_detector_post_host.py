"""The detector's output side without a device: the twin (tests/detpost_ref.py) against vectors derived by hand from DESIGN.md section
21, the twin's per-image outputs through the existing io_formats.make_detections against the twin's own end-to-end collection, and the
argument checks of cosypose_amd/detector.py, which must refuse a bad call before the library is even loaded."""
import math

import numpy as np
import pytest
import torch

import detpost_ref as ref
from cosypose_amd import detector
from cosypose_amd.io_formats import make_detections


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
#                 box 0            IoU with 0: 50/100      60/100          50/150 (and 25/125 with box 1)
NMS_BOXES = [[0, 0, 10, 10], [0, 0, 10, 5], [0, 0, 10, 6], [5, 0, 15, 10]]
NMS_SCORES = [0.9, 0.8, 0.7, 0.6]


def test_twin_iou_of_the_hand_boxes_is_exact():
    b = ref.f32(NMS_BOXES)
    assert float(ref.iou(b[0], b[1])) == 0.5
    assert float(ref.iou(b[0], b[2])) == np.float32(0.6)
    assert float(ref.iou(b[0], b[3])) == np.float32(50) / np.float32(150)
    assert float(ref.iou(b[1], b[3])) == np.float32(0.2)


def test_twin_nms_suppresses_strictly_above_the_threshold():
    # 0.5 is not > 0.5: box 1 stays; 0.6 goes; 1/3 stays
    assert ref.nms(NMS_BOXES, NMS_SCORES, 0.5).tolist() == [0, 1, 3]
    assert ref.nms(NMS_BOXES, NMS_SCORES, 0.49).tolist() == [0, 3]
    assert ref.nms(NMS_BOXES, NMS_SCORES, 0.5, max_keep=2).tolist() == [0, 1]
    assert ref.nms(np.zeros((0, 4)), [], 0.5).tolist() == []


def test_twin_nms_visits_equal_scores_lower_index_first():
    boxes = [[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]]
    assert ref.nms(boxes, [0.5, 0.5, 0.5], 0.5).tolist() == [0, 2]
    assert ref.nms(boxes, [0.5, 0.7, 0.5], 0.5).tolist() == [1, 2]


def test_twin_label_shift_keeps_identical_boxes_of_different_classes():
    boxes = [[2, 3, 12, 13], [2, 3, 12, 13], [2, 3, 12, 13]]
    assert ref.batched_nms(boxes, [0.9, 0.8, 0.7], [1, 2, 1], 0.5).tolist() == [0, 1]
    assert ref.batched_nms(boxes, [0.9, 0.8, 0.7], [1, 1, 1], 0.5).tolist() == [0]
    assert ref.batched_nms(np.zeros((0, 4)), [], [], 0.5).tolist() == []


# ---- decode ------------------------------------------------------------------------------------------------------------------------
def test_twin_decode_clamps_the_size_deltas():
    # proposal 16 x 16 at the origin, C = 2: r2 / 5 = 6 > log(1000/16), so the width is 16 * 1000/16 = 1000 around cx = 8; dy = 5/10 of h moves the centre from 8 to 16
    reg = np.zeros((1, 8), np.float32)
    reg[0, 4:] = [0, 5, 30, 0]
    box = ref.decode(reg, [[0, 0, 16, 16]])[0, 1].numpy()
    assert abs(box[0] - (8 - 500)) < 1e-3 and abs(box[2] - (8 + 500)) < 1e-3
    assert box[1] == 8 and box[3] == 24
    assert np.array_equal(ref.decode(reg, [[0, 0, 16, 16]])[0, 0].numpy(), [0, 0, 16, 16])          # zero deltas: the proposal
    clipped = ref.clip(ref.decode(reg, [[0, 0, 16, 16]]), (37, 53))[0, 1].numpy()
    assert clipped.tolist() == [0, 8, 53, 24]


def test_twin_postprocess_applies_threshold_small_box_test_and_cut():
    logits, reg, props = ref.head_case(3, [70, 1], 5, (37, 53))
    s64 = ref.scores64(logits)[:, 1:]
    assert 0.05 < float(s64[1, 0]) < 0.05 + 1e-3                              # the planted near-threshold score is a candidate
    assert int(((s64 - 0.05).abs() < 1e-4).sum()) == 0                        # ... and nothing is too close to call
    full = ref.postprocess(logits, reg, props, [(37, 53)] * 2, [(24, 40)] * 2, detections_per_img=1000)
    cut = ref.postprocess(logits, reg, props, [(37, 53)] * 2, [(24, 40)] * 2, detections_per_img=3)
    assert len(full[0]['scores']) > 3 and len(cut[0]['scores']) == 3
    assert np.array_equal(full[0]['boxes'][:3], cut[0]['boxes']) and np.all(np.diff(full[0]['scores']) <= 0)
    pairs = set(zip(full[0]['proposal'].tolist(), full[0]['labels'].tolist()))
    assert (69, 1) not in pairs                                               # score 1, but zero width after the clip
    assert (0, 1) in pairs                                                    # the clamped decode fills the image
    got = full[0]['boxes_net'][[p == 0 and l == 1 for p, l in zip(full[0]['proposal'], full[0]['labels'])]][0]
    assert got[0] == 0 and got[2] == 53
    assert np.array_equal(full[0]['boxes'][:, 0], full[0]['boxes_net'][:, 0] * (np.float32(40) / np.float32(53)))
    assert np.array_equal(full[0]['boxes'][:, 3], full[0]['boxes_net'][:, 3] * (np.float32(24) / np.float32(37)))


# ---- paste -------------------------------------------------------------------------------------------------------------------------
def test_twin_paste_of_a_constant_mask_half_outside_the_frame():
    # M = 4, scale 6/4: box x -6.5 .. 6 -> xc -0.25, half width 6.25 * 1.5 = 9.375 -> -9.625 .. 9.125 -> TRUNCATED to -9 .. 9 (floor: -10),
    # w = 19; y 2 .. 10 -> yc 6, half height 6 -> 0 .. 12, h = 13.  Frame 12 x 16: columns 0 .. min(9 + 1, 16) - 1 = 9 and rows 0 .. 11 take
    # interpolated values.  The padded mask is the outer product of the profile 0 1 1 1 1 0, so the value is vx(x) vy(y) with
    # v(s) = s on [0,1], 1 on [1,4], 5 - s on [4,5], s = 6/n (i + 1/2) - 1/2 clamped at 0.
    assert ref.box_pixels([-6.5, 2, 6, 10], 4) == (-9, 0, 9, 12)
    logits = np.full((1, 2, 4, 4), 20, np.float32)
    logits[0, 0] = -20
    values, inside = ref.paste_values(logits, [[-6.5, 2, 6, 10]], [1], (12, 16))
    want_inside = np.zeros((12, 16), bool)
    want_inside[0:12, 0:10] = True
    assert np.array_equal(inside[0].numpy(), want_inside)

    def profile(i, n):
        s = max(6 / n * (i + 0.5) - 0.5, 0)
        return min(s, 1, max(5 - s, 0))
    want = np.array([[profile(y - 0, 13) * profile(x + 9, 19) if x < 10 else 0 for x in range(16)] for y in range(12)])
    assert np.abs(values[0].numpy() - want).max() < 1e-5
    # value > 0: columns 2 .. 16 of the box = -7 .. 7 of the frame, rows 1 .. 11: an exact rectangle
    mask0 = ref.paste_masks(logits, [[-6.5, 2, 6, 10]], [1], (12, 16), mask_th=0.0)[0]
    rect = np.zeros((12, 16), bool)
    rect[1:12, 0:8] = True
    assert np.array_equal(mask0, rect)
    # value > 0.5: 6/19 (i + 1/2) - 1/2 > 1/2 from i = 3 on, < 4.5 up to i = 15: columns -6 .. 6; rows 2 .. 10, but the corner where both ramp
    assert abs(want - 0.5).min() > 1e-3
    assert np.array_equal(ref.paste_masks(logits, [[-6.5, 2, 6, 10]], [1], (12, 16), mask_th=0.5)[0], want > 0.5)
    assert ref.paste_masks(logits, [[-6.5, 2, 6, 10]], [0], (12, 16), mask_th=0.5).sum() == 0        # channel 0 holds -20


def test_twin_paste_outside_and_one_pixel_boxes():
    logits = np.full((2, 1, 4, 4), 20, np.float32)
    values, inside = ref.paste_values(logits, [[40, 40, 50, 50], [3.2, 4.1, 3.4, 4.3]], [0, 0], (12, 16))
    assert not inside[0].any()
    assert inside[1].sum() == 1 and inside[1, 4, 3]                            # 3.3 -+ 0.15 and 4.2 -+ 0.15 truncate to one pixel
    assert abs(float(values[1, 4, 3]) - 1.0) < 1e-6                            # the centre of the padded mask


# ---- filters -----------------------------------------------------------------------------------------------------------------------
def per_image_case():
    mk = lambda boxes, scores, labels: dict(boxes=np.asarray(boxes, np.float32), boxes_net=np.asarray(boxes, np.float32) * 2,
                                            scores=np.asarray(scores, np.float32), labels=np.asarray(labels, np.int64))
    return [mk([[1, 1, 5, 5], [2, 2, 8, 8], [0, 0, 3, 3]], [0.9, 0.5, 0.25], [1, 2, 1]),
            mk([[4, 4, 9, 9], [1, 2, 3, 4]], [0.95, 0.5], [2, 3])]


NAMES = {1: 'obj_a', 2: 'obj_b', 3: 'obj_c'}


def test_twin_one_instance_per_class_spans_the_batch():
    got = ref.get_detections(per_image_case(), NAMES, one_instance_per_class=True)
    # obj_b: 0.95 of frame 1 beats 0.5 of frame 0; obj_a: 0.9 of frame 0; obj_c: 0.5 of frame 1; by descending score
    assert got['rows'] == [(1, 0), (0, 0), (1, 1)]
    assert got['label'].tolist() == ['obj_b', 'obj_a', 'obj_c'] and got['batch_im_id'].tolist() == [1, 0, 1]
    th = ref.get_detections(per_image_case(), NAMES, detection_th=0.5)
    assert th['rows'] == [(0, 0), (1, 0)]                                      # 0.5 is not > 0.5
    th = ref.get_detections(per_image_case(), NAMES, detection_th=0.49)
    assert th['rows'] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    both = ref.get_detections(per_image_case(), NAMES, detection_th=0.5, one_instance_per_class=True)
    assert both['rows'] == [(1, 0), (0, 0)]


@pytest.mark.parametrize('detection_th', [None, 0.3])
@pytest.mark.parametrize('one_instance_per_class', [False, True])
@pytest.mark.parametrize('output_masks', [False, True])
def test_twin_collection_equals_make_detections_on_the_twins_per_image_outputs(detection_th, one_instance_per_class, output_masks):
    C, M, frame, net = 4, 14, (24, 40), (37, 53)
    logits, reg, props = ref.head_case(5, [40, 25], C, net)
    logits = (logits * 0.25).astype(np.float32)                    # flatter softmaxes: scores on both sides of detection_th = 0.3
    per_image = ref.postprocess(logits, reg, props, [net] * 2, [frame] * 2, detections_per_img=100)
    names = {c: f'obj_{c:06d}' for c in range(1, C)}
    all_logits = [ref.smooth_mask_logits(11 + b, len(out['scores']), C, M) for b, out in enumerate(per_image)]

    def mask_head(boxes_net, batch_im_id):                                     # the logits of a detection follow it through the filters
        rows = [int(np.flatnonzero((per_image[b]['boxes_net'] == bn).all(1))[0]) for bn, b in zip(boxes_net, batch_im_id)]
        return np.stack([all_logits[b][j] for b, j in zip(batch_im_id, rows)])
    want = ref.get_detections(per_image, names, mask_head, frame, detection_th, one_instance_per_class, output_masks, 0.8)
    fed = [dict(boxes=out['boxes'], labels=[names[int(l)] for l in out['labels']], scores=out['scores'],
                masks=ref.paste_values(all_logits[b], out['boxes'], out['labels'], frame)[0][:, None]) for b, out in enumerate(per_image)]
    got = make_detections(fed, device='cpu', detection_th=detection_th, one_instance_per_class=one_instance_per_class,
                          output_masks=output_masks, mask_th=0.8)
    assert len(got.infos) == len(want['score']) > 0
    assert detection_th is None or one_instance_per_class or len(got.infos) < sum(len(o['scores']) for o in per_image)
    assert got.infos['batch_im_id'].tolist() == want['batch_im_id'].tolist() and got.infos['label'].tolist() == want['label'].tolist()
    assert np.array_equal(got.infos['score'].values, want['score'])
    assert np.array_equal(got.bboxes.numpy(), want['bboxes'])
    assert hasattr(got, 'masks') == output_masks
    if output_masks:
        assert got.masks.dtype == torch.bool and np.array_equal(got.masks.numpy(), want['masks']) and want['masks'].any()


# ---- the wrappers' checks ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(detector._lib, 'lib', boom)


def test_wrappers_refuse_bad_arguments_before_loading_the_library(no_library):
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match='ROCm device'):
        detector.nms(f(3, 4), f(3), 0.5)                                       # host tensors
    with pytest.raises(ValueError, match='boxes must be'):
        detector.nms(f(3, 5), f(3), 0.5)
    with pytest.raises(ValueError, match='float32'):
        detector.nms(f(3, 4).double(), f(3), 0.5)
    with pytest.raises(ValueError, match='scores must be'):
        detector.nms(f(3, 4), f(4), 0.5)
    with pytest.raises(ValueError, match='idxs must be int32 or int64'):
        detector.batched_nms(f(3, 4), f(3), f(3), 0.5)
    with pytest.raises(ValueError, match='exceed the cap'):
        detector.nms(f(detector.MAX_CANDIDATES + 1, 4), f(detector.MAX_CANDIDATES + 1), 0.5)
    args = dict(net_sizes=[(37, 53)], original_sizes=[(24, 40)])
    with pytest.raises(ValueError, match='ROCm device'):
        detector.postprocess_detections(f(7, 3), f(7, 12), [f(7, 4)], **args)
    with pytest.raises(ValueError, match='box_regression must be'):
        detector.postprocess_detections(f(7, 3), f(7, 11), [f(7, 4)], **args)
    with pytest.raises(ValueError, match='class_logits must be'):
        detector.postprocess_detections(f(6, 3), f(7, 12), [f(7, 4)], **args)
    with pytest.raises(ValueError, match='need `counts`'):
        detector.postprocess_detections(f(7, 3), f(7, 12), f(7, 4), **args)
    with pytest.raises(ValueError, match='net_sizes must hold one'):
        detector.postprocess_detections(f(7, 3), f(7, 12), [f(7, 4)], net_sizes=[(37, 53)] * 2)
    with pytest.raises(ValueError, match='background column'):
        detector.postprocess_detections(f(7, 1), f(7, 4), [f(7, 4)], **args)
    with pytest.raises(ValueError, match='mask_logits must be'):
        detector.paste_masks(f(2, 3, 14, 13), f(2, 4), torch.zeros(2, dtype=torch.int64), (24, 40))
    with pytest.raises(ValueError, match='side 1 <= M'):
        detector.paste_masks(f(2, 3, 63, 63), f(2, 4), torch.zeros(2, dtype=torch.int64), (24, 40))
    with pytest.raises(ValueError, match='ROCm device'):
        detector.paste_masks(f(2, 3, 14, 14), f(2, 4), torch.zeros(2, dtype=torch.int64), (24, 40))
    with pytest.raises(ValueError, match='labels must be'):
        detector.paste_masks(f(2, 3, 14, 14), f(2, 4), torch.zeros(3, dtype=torch.int64), (24, 40))
    with pytest.raises(ValueError, match='ROCm device'):
        detector.detections_from_heads(f(7, 3), f(7, 12), [f(7, 4)], [(37, 53)], [(24, 40)], {1: 'a', 2: 'b'})


def test_lazy_names():
    import cosypose_amd
    for name in ('nms', 'batched_nms', 'postprocess_detections', 'paste_masks', 'detections_from_heads'):
        assert getattr(cosypose_amd, name) is getattr(detector, name)
    assert detector._lib.EXPORTS.count('cosy_paste_masks') == 1


# ---- the twin's additions for tests/test_detpost_kernels.py --------------------------------------------------------------------------
def integer_nms_case(N, seed=0):
    """test_detector_post.py's nms_case, restated here (that module needs a device to import)"""
    rng = np.random.RandomState(seed + N)
    x1, y1 = rng.randint(0, 40, N), rng.randint(0, 40, N)
    boxes = np.stack([x1, y1, x1 + rng.randint(1, 21, N), y1 + rng.randint(1, 21, N)], 1).astype(np.float32)
    if N >= 2:
        boxes[0], boxes[1] = [0, 0, 10, 10], [0, 0, 10, 5]
    if N >= 65:
        boxes[63], boxes[64] = [30, 30, 50, 40], [30, 30, 50, 35]
    return boxes, (rng.randint(1, 17, N) / 16).astype(np.float32), rng.randint(0, 3, N).astype(np.int64)


@pytest.mark.parametrize('N', [0, 1, 2, 63, 64, 65, 130])
def test_vectorised_nms_equals_the_loop_on_the_integer_cases(N):
    boxes, scores, labels = integer_nms_case(N)
    for max_keep in (None, 7):
        assert ref.nms_fast(boxes, scores, 0.5, max_keep).tolist() == ref.nms(boxes, scores, 0.5, max_keep).tolist()
        assert ref.batched_nms_fast(boxes, scores, labels, 0.5, max_keep).tolist() == ref.batched_nms(boxes, scores, labels, 0.5, max_keep).tolist()


@pytest.mark.parametrize('N', [129, 400])
def test_vectorised_nms_equals_the_loop_on_random_float_boxes(N):
    boxes, scores, labels = ref.nms_clustered_case(N)
    for thr in (0.5, 0.3, 0.0, float('nan')):
        want = ref.nms(boxes, scores, thr)
        assert ref.nms_fast(boxes, scores, thr).tolist() == want.tolist()
    assert 0 < len(ref.nms(boxes, scores, 0.5)) < N
    assert ref.batched_nms_fast(boxes, scores, labels, 0.5).tolist() == ref.batched_nms(boxes, scores, labels, 0.5).tolist()
    lb, ls, ll = ref.nms_label_case(N=N)                                    # shifts of 4e6: the rounded coordinates
    assert ref.batched_nms_fast(lb, ls, ll, 0.5).tolist() == ref.batched_nms(lb, ls, ll, 0.5).tolist()
    lb[N // 3, 1] = np.nan                                                  # one NaN: every shift is NaN
    assert ref.batched_nms_fast(lb, ls, ll, 0.5).tolist() == ref.batched_nms(lb, ls, ll, 0.5).tolist() == ref.visiting_order(ls)


def test_vectorised_nms_at_the_largest_size_takes_seconds():
    import time
    boxes, scores, _ = ref.nms_clustered_case(16384)
    t0 = time.time()
    keep = ref.nms_fast(boxes, scores, 0.5)
    took = time.time() - t0
    print(f'N=16384: kept {len(keep)} in {took:.2f} s')
    assert 100 < len(keep) < 2000 and took < 20


def test_decode64_agrees_with_the_float32_twin_within_its_bound():
    logits, reg, props = ref.head_case(9, [70, 40], 5, (37, 53))
    want32 = ref.decode(reg, np.concatenate(props)).numpy().astype(np.float64)
    got, bound = ref.decode64(reg, np.concatenate(props))
    frac = np.abs(want32 - got) / bound
    print(f'float32 twin against decode64: worst {frac.max():.3f} of the bound')
    assert got.shape == bound.shape == (110, 5, 4) and frac.max() <= 1
    # the bound is a few units of float32 rounding of the quantities involved, not a loose figure: at most 16 u of their sum
    reg64 = reg.reshape(110, 5, 4).astype(np.float64)
    assert (bound <= 16 * ref.U32 * (np.abs(got).max(-1, keepdims=True) + 25 + 1000 * (reg64[..., 2:].max(-1, keepdims=True) >= 20))).all()
    # by hand: proposal (0, 0, 16, 16), deltas (0, 5, 30, 0): cx 8 +- 500 through the clamp, cy 8 + 0.5 * 16 = 16 +- 8
    hand = np.zeros((1, 8), np.float32)
    hand[0, 4:] = [0, 5, 30, 0]
    box, b = ref.decode64(hand, [[0, 0, 16, 16]])
    assert np.abs(box[0, 1] - [8 - 500, 8, 8 + 500, 24]).max() < 1e-9 and np.array_equal(box[0, 0], [0, 0, 16, 16])
    assert np.array_equal(ref.clip64(box, (37, 53))[0, 1], [0, 8, 53, 24])
    # x: |x| 508 + |pcx| 8 + 0 + 8 + 8 + (4.135 + 4) / 2 * 1000 = 4599.6 units of 2^-24
    assert abs(b[0, 1, 2] / ref.U32 - (508 + 8 + 8 + 8 + 0.5 * (ref.XFORM_CLIP + 4) * 1000)) < 5


def test_paste_value64_equals_the_interpolating_twin_in_float64():
    boxes = np.array([[10.3, 8.2, 30.7, 25.9], [-5.5, 10, 8, 20], [20, -6.2, 35, 7.5], [45, 12, 60.4, 30], [12, 30, 28, 44.3],
                      [70, 50, 90, 60], [-30, -30, -10, -5], [3.2, 4.1, 3.4, 4.3], [-20, -15, 80, 60]], np.float32)    # PASTE_BOXES of the GPU suite
    for M in (14, 28):
        for frame in ((37, 53), (24, 40), (130, 128)):
            H, W = frame
            b = boxes * np.array([W / 53, H / 37, W / 53, H / 37], np.float32)
            b[7] = boxes[7]
            logits = ref.smooth_mask_logits(M, len(b), 3, M)
            labels = np.arange(len(b)) % 3
            want, want_inside = ref.paste_values(logits, b, labels, frame, torch.float64)
            got, inside = ref.paste_values64(logits, b, labels, frame)
            assert np.array_equal(inside, want_inside.numpy())
            err = np.abs(got - want.numpy()).max()
            assert err <= 1e-12, (M, frame, err)


def test_box_pixels_for_non_finite_huge_and_inverted_boxes():
    nan, inf = float('nan'), float('inf')
    assert ref.box_pixels([nan, nan, nan, nan], 14) == (0, 0, 0, 0)
    assert ref.box_pixels([-1e12, -1e12, 1e12, 1e12], 14) == (-2 ** 29, -2 ** 29, 2 ** 29, 2 ** 29)
    assert ref.box_pixels([0, 0, inf, inf], 14) == (0, 0, 2 ** 29, 2 ** 29)        # xc = inf, wh = inf: inf - inf = NaN -> 0, inf + inf -> 2^29
    assert ref.box_pixels([nan, 5, 20, 15], 14)[::2] == (0, 0)
    # inverted in x: xc 20, wh -10 * 16/14 = -11.43: 31.43 -> 31 and 8.57 -> 8; y as usual: 12.5 -+ 7.5 * 16/14 = 3.93, 21.07
    assert ref.box_pixels([30, 5, 10, 20], 14) == (31, 3, 8, 21)
    values, inside = ref.paste_value64(np.full((1, 14, 14), 3.0, np.float32), [30, 5, 10, 20], 0, (24, 40))
    assert not inside.any() and not values.any()                                   # bx1 > bx2: an empty region
    assert ref.box_pixels([-6.5, 2, 6, 10], 4) == (-9, 0, 9, 12)                   # finite boxes as before
    # the all-NaN box: pixel (0, 0) of a (1, 1) upsample: s = 16/1 * 0.5 - 0.5 = 7.5 on both axes, the mean of the four centre taps
    logits = ref.smooth_mask_logits(3, 1, 1, 14)
    values, inside = ref.paste_value64(logits[0], [nan] * 4, 0, (24, 40))
    prob = 1 / (1 + np.exp(-logits[0, 0].astype(np.float64)))
    assert inside.sum() == 1 and inside[0, 0] and abs(values[0, 0] - prob[6:8, 6:8].mean()) < 1e-15
    # the clamped box: 2^30 + 1 pixels a side, the frame sits at its centre: one value to 1e-6
    values, inside = ref.paste_value64(logits[0], [-1e12, -1e12, 1e12, 1e12], 0, (24, 40))
    assert inside.all() and np.abs(values - prob[6:8, 6:8].mean()).max() < 1e-5 * 14


def test_new_paste_inputs_stay_inside_the_exclusion_cap():
    """at most 0.1 % of a mask's in-box pixels within 1e-5 of mask_th, on the reference alone, for every input of the GPU suite's paste group"""
    cases = ref.paste_edge_cases()
    assert set(cases) >= {'M1', 'M2', 'M61', 'M62', 'chunks', 'one_pixel_frame', 'one_row', 'one_column_wide', 'one_column_scalar', 'alignment',
                          'boxes', 'labels', 'mask_th'}
    for name, c in cases.items():
        v64, inside = ref.paste_values64(c['logits'], c['boxes'], c['labels'], c['frame'])
        in_box = inside.reshape(len(v64), -1).sum(1)
        for th in c['mask_ths']:
            close = (np.abs(v64 - th) <= 1e-5) & inside
            assert (close.reshape(len(v64), -1).sum(1) <= 1e-3 * in_box).all(), (name, th)
    # the rows the chunk boxes were built for (a workgroup of the (260, 128) frame owns rows 0-127, 128-255, 256-259)
    c = cases['chunks']
    rows = [ref.box_pixels(b, 14)[1::2] for b in c['boxes']]
    assert rows == [(128, 151), (98, 127), (135, 204), (3, 275), (256, 259), (127, 127), (128, 128)]
    assert [ref.box_pixels(b, 28)[0::2] for b in cases['one_row']['boxes']][2] == (1023, 1024)      # two pixels across a workgroup seam
    # mask_th group: every in-box value is strictly between 1e-4 and 0.75, the outside is exactly 0
    c = cases['mask_th']
    v64, inside = ref.paste_values64(c['logits'], c['boxes'], c['labels'], c['frame'])
    assert v64[inside].min() > 1e-4 and v64[inside].max() < 0.75 and not v64[~inside].any() and not inside[3].any() and inside[:3].any((1, 2)).all()
    assert ref.paste_masks(c['logits'], c['boxes'], c['labels'], c['frame'], -0.5).all()            # 0 > -0.5: the outside is true too
    assert np.array_equal(ref.paste_masks(c['logits'], c['boxes'], c['labels'], c['frame'], 0.0), inside)
    assert not ref.paste_masks(c['logits'], c['boxes'], c['labels'], c['frame'], float('nan')).any()


def test_wrapper_refuses_the_key_limits_before_loading_the_library(no_library):
    f = lambda *s: torch.empty(*s)
    with pytest.raises(ValueError, match='2048 images exceed the limit of 2047'):
        detector.postprocess_detections(f(2048, 2), f(2048, 8), f(2048, 4), [(37, 53)] * 2048, counts=[1] * 2048)
    with pytest.raises(ValueError, match='C = 4097 classes exceed the limit of 4096'):
        detector.postprocess_detections(f(1, 4097), f(1, 4 * 4097), [f(1, 4)], [(37, 53)])
    with pytest.raises(ValueError, match=r'exceeds the limit of 2\^21'):
        detector.postprocess_detections(f(2 ** 21 + 1, 2), f(2 ** 21 + 1, 8), [f(2 ** 21 + 1, 4)], [(37, 53)])
    with pytest.raises(ValueError, match=r'exceeds the limit of 2\^21'):
        detector.postprocess_detections(f(2 ** 19 + 1, 5), f(2 ** 19 + 1, 20), [f(2 ** 19 + 1, 4)], [(37, 53)])
    with pytest.raises(ValueError, match='ROCm device'):                       # at the limits the call goes on to the next check
        detector.postprocess_detections(f(2047, 2), f(2047, 8), f(2047, 4), [(37, 53)] * 2047, counts=[1] * 2047)


def test_score_key_orders_scores_descending():
    # the sort key of csrc/kernels_detpost.hip: positive float32 bits order as the values do
    s = np.array([0.05000001, 0.0500001, 0.3, 0.99999994, 1.0], np.float32)
    key = 0x7fffffff - s.view(np.int32).astype(np.int64)
    assert np.all(np.diff(key) < 0) and key.min() >= 0 and key.max() < 2 ** 31
    assert math.isclose(ref.XFORM_CLIP, 4.135166556742356)

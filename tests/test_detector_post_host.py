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


def test_score_key_orders_scores_descending():
    # the sort key of csrc/kernels_detpost.hip: positive float32 bits order as the values do
    s = np.array([0.05000001, 0.0500001, 0.3, 0.99999994, 1.0], np.float32)
    key = 0x7fffffff - s.view(np.int32).astype(np.int64)
    assert np.all(np.diff(key) < 0) and key.min() >= 0 and key.max() < 2 ** 31
    assert math.isclose(ref.XFORM_CLIP, 4.135166556742356)

"""CPU: the twin of the detector's training side (tests/dettrain_ref.py) against hand-derived vectors, the argument
checks of cosypose_amd/detector_train.py, which must refuse a bad call before the library is even loaded, and the ABI of the new entry points."""
import math
import os
import re

import numpy as np
import pytest
import torch

import dettrain_ref as ref
from cosypose_amd import detector, detector_train as dt

f32 = np.float32
LN2 = math.log(2.0)
NAMES = ('cosy_dt_match', 'cosy_dt_sample', 'cosy_dt_encode', 'cosy_dt_rpn_loss', 'cosy_dt_roi_candidates', 'cosy_dt_roi_gather',
         'cosy_dt_fastrcnn_loss', 'cosy_dt_mask_loss')


# ---- the twin against hand-derived vectors ---------------------------------------------------------------------------------------------
def test_twin_match_restores_the_original_argmax():
    # IoU rows (ground truth) x columns (anchor):  g0 = 10 x 10: [1, 0.5];  g1 = 10 x 2 inside both: [20 / 100, 20 / 50] = [0.2, 0.4]
    gt = np.array([[0, 0, 10, 10], [0, 3, 10, 5]], f32)
    anchors = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], f32)
    assert ref.box_iou(gt, anchors).tolist() == [[1.0, 0.5], [f32(0.2), f32(0.4)]]
    m, v = ref.match(gt, anchors, 0.7, 0.3, False)
    assert m.tolist() == [0, -2] and v.tolist() == [1.0, 0.5]                  # anchor 1: 0.3 <= 0.5 < 0.7 is "between"
    # anchor 1 is the best anchor of g1 (0.4 > 0.2): it gets back ITS argmax, g0 -- not g1
    m, _ = ref.match(gt, anchors, 0.7, 0.3, True)
    assert m.tolist() == [0, 0]
    assert ref.labels_of(np.array([0, -1, -2, 1]), None).tolist() == [1, 0, -1, 1]
    assert ref.labels_of(np.array([0, -1, -2, 1]), [7, 9]).tolist() == [7, 0, -1, 9]


def test_twin_match_a_ground_truth_without_overlap_restores_every_zero():
    gt = np.array([[0, 0, 10, 10], [100, 100, 110, 110]], f32)
    anchors = np.array([[0, 0, 10, 10], [20, 20, 30, 30]], f32)
    assert ref.match(gt, anchors, 0.7, 0.3, False)[0].tolist() == [0, -1]
    # best[g1] == 0: both anchors have IoU 0 with g1 and are restored; anchor 1's argmax over [0, 0] is the lowest g
    assert ref.match(gt, anchors, 0.7, 0.3, True)[0].tolist() == [0, 0]
    # two identical ground truths: the lower index; a zero-area pair gives 0 / 0 = NaN, which counts as 0
    assert ref.match(gt[[0, 0]], anchors, 0.7, 0.3, False)[0].tolist() == [0, -1]
    z = np.array([[5, 5, 5, 5]], f32)
    assert ref.box_iou(z, z).tolist() == [[0.0]]
    # padding rows take no part, in the restore either
    m, v = ref.match(gt, np.concatenate([anchors, np.zeros((1, 4), f32)]), 0.5, 0.5, True, n_real=2)
    assert m.tolist() == [0, 0, -3] and v.tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize('P,N,want', [(3, 5, (2, 2)),      # n_pos = int(bs frac), n_neg = bs - n_pos
                                      (1, 5, (1, 3)),      # n_pos = P
                                      (3, 1, (2, 1)),      # n_neg = N
                                      (1, 1, (1, 1)), (0, 9, (0, 4)), (9, 0, (2, 0)), (0, 0, (0, 0))])
def test_twin_sampler_counts(P, N, want):
    labels = np.array([1] * P + [0] * N + [-1] * 3)
    samp, pos = ref.sample(labels, np.arange(len(labels))[::-1].copy(), 4, 0.5)
    assert (len(pos), len(samp) - len(pos)) == want
    assert (labels[samp] >= 0).all() and (np.diff(samp) > 0).all()


def test_twin_sampler_takes_the_smallest_keys_lower_index_first():
    labels = np.array([1, 0, 1, 1, 0, -1, 0, 1])
    keys = np.array([5, 2, 5, 1, 2, 0, 2, 5])
    samp, pos = ref.sample(labels, keys, 4, 0.5)
    assert pos.tolist() == [0, 3]                                              # key 1, then the lowest index among the 5s
    assert samp.tolist() == [0, 1, 3, 4]                                       # negatives: all keys 2 -> indices 1 and 4


def test_twin_encode():
    got = ref.encode([[0, 0, 20, 10]], [[0, 0, 10, 10]], ref.ROI_WEIGHTS)[0]
    assert got[0] == 5 and got[1] == 0 and got[3] == 0 and abs(got[2] - 5 * LN2) < 1e-6
    t64, bound = ref.encode([[0, 0, 20, 10]], [[0, 0, 10, 10]], ref.ROI_WEIGHTS, np.float64)
    assert t64[0, 2] == 5 * LN2 and (bound > 0).all() and (bound < 1e-5).all()
    with np.errstate(all='ignore'):
        zero = ref.encode([[0, 0, 20, 10]], [[3, 0, 3, 10]], ref.RPN_WEIGHTS)[0]
    assert np.isinf(zero[0]) and zero[1] == 0 and np.isinf(zero[2])


def test_twin_loss_terms():
    assert ref.bce64(0, 1) == LN2 and ref.bce64(0, 0) == LN2
    assert abs(ref.bce64(100, 1) - math.exp(-100)) < 1e-50 and ref.bce64(100, 0) == 100 and np.isfinite(ref.bce64(-1e4, 1))
    assert ref.sigmoid64(0) == 0.5 and ref.sigmoid64(-1e4) == 0 and ref.sigmoid64(1e4) == 1
    assert [float(v) for v in ref.smooth_l1_64(0.5, 1.0)] == [0.125, 0.5]
    assert [float(v) for v in ref.smooth_l1_64(-2.0, 1.0)] == [1.5, -1.0]
    assert [float(v) for v in ref.smooth_l1_64(1.0, 1.0)] == [0.5, 1.0]
    assert [float(v) for v in ref.smooth_l1_64(-0.25, 0)] == [0.25, -1.0]


def test_twin_rpn_loss_of_one_anchor():
    # one cell, one anchor [-16, -16, 16, 16] equal to the ground truth: positive, targets 0, N_s = 1
    obj, dl = [np.zeros((1, 1, 1, 1), f32)], [np.array([1, -2, 0, 0.5], f32).reshape(1, 4, 1, 1)]
    out = ref.rpn_loss(obj, dl, [np.array([[-16, -16, 16, 16]], f32)], (32, 32), ((32,),), (1.0,), np.zeros((1, 1), np.int64))
    assert out['matched'].tolist() == [[0]] and out['n_sampled'] == 1
    assert out['losses'] == dict(loss_objectness=LN2, loss_rpn_box_reg=3.5)
    assert out['grad_objectness'][0].reshape(-1).tolist() == [-0.5]
    assert out['grad_deltas'][0].reshape(-1).tolist() == [1, -1, 0, 1]


def test_twin_fastrcnn_loss():
    z = np.zeros((3, 2), f32)
    d = np.zeros((3, 8), f32)
    d[0, 4:] = [0.5, 2, 0, -3]
    out = ref.fastrcnn_loss(z, d, [1, 0, -1], np.zeros((3, 4), f32))
    assert out['n'] == 2                                                       # the background row counts, the padding row does not
    assert out['losses'] == dict(loss_classifier=LN2, loss_box_reg=(0.125 + 1.5 + 0 + 2.5) / 2)
    assert out['grad_logits'].tolist() == [[0.25, -0.25], [-0.25, 0.25], [0, 0]]
    assert out['grad_box'][0].tolist() == [0, 0, 0, 0, 0.25, 0.5, 0, -0.5] and not out['grad_box'][1:].any()


def test_twin_mask_targets_and_loss():
    mask = np.array([[[1, 2], [3, 4]]], np.uint8)
    assert ref.adaptive_grid(0, 28, 28) == 1 and ref.adaptive_grid(0, 28.5, 28) == 2 and ref.adaptive_grid(3, 3.2, 28) == 1
    assert ref.adaptive_grid(0, 1e30, 28) == ref.MAX_GRID
    assert ref.mask_targets(mask, [[0, 0, 1, 1]], [0], 1).tolist() == [[[2.5]]]         # g = 1: the sample at (0.5, 0.5)
    # g = 2: samples at 0.5 and 1.5; 1.5 >= size - 1 is the last pixel alone: 2.5, 3 (column 1 of both rows), 3.5, 4
    assert ref.mask_targets(mask, [[0, 0, 2, 2]], [0], 1).tolist() == [[[3.25]]]
    assert ref.mask_targets(mask, [[0, 0, 2, 2]], [1], 1).tolist() == [[[0.0]]]          # a matched index no mask has
    loss, bound, grad, n = ref.mask_loss(np.zeros((2, 3, 1, 1), f32), [2, 1], np.array([[[1.0]], [[0.0]]], f32), np.array([True, False]))
    assert loss == LN2 and n == 1 and 0 < bound < 1e-6
    assert grad[0, 2, 0, 0] == -0.5 and np.count_nonzero(grad) == 1
    assert ref.mask_loss(np.zeros((2, 3, 1, 1), f32), [2, 1], np.zeros((2, 1, 1), f32), np.array([False, False]))[0] == 0.0


# ---- the wrappers' checks ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(detector._lib, 'lib', boom)


def _target(G=2, H=24, W=40):
    return dict(boxes=torch.zeros(G, 4), labels=torch.ones(G, dtype=torch.int64), masks=torch.zeros(G, H, W, dtype=torch.uint8))


def test_wrappers_refuse_bad_arguments_before_loading_the_library(no_library):
    f = lambda *s: torch.zeros(*s)
    gt = [f(2, 4), f(3, 4)]
    with pytest.raises(ValueError, match='ROCm device'):
        dt.match_boxes(gt, f(2, 5, 4), 0.5, 0.5)
    with pytest.raises(ValueError, match='holds no ground truth'):
        dt.match_boxes([f(2, 4), f(0, 4)], f(2, 5, 4), 0.5, 0.5)
    with pytest.raises(ValueError, match=f'the limit is {dt.MAX_GT} per image'):
        dt.match_boxes([f(dt.MAX_GT + 1, 4)], f(1, 5, 4), 0.5, 0.5)
    with pytest.raises(ValueError, match='must not exceed high_threshold'):
        dt.match_boxes(gt, f(2, 5, 4), 0.3, 0.7)
    with pytest.raises(ValueError, match=r'candidates must be \(2,\*,4\)'):
        dt.match_boxes(gt, f(3, 5, 4), 0.5, 0.5)
    with pytest.raises(ValueError, match='counts go with a tensor'):
        dt.match_boxes(gt, dt.AnchorGrid([(5, 7)], (40, 56), ((32,),)), 0.7, 0.3, True, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='gt_labels must hold one tensor per image'):
        dt.match_boxes(gt, f(2, 5, 4), 0.5, 0.5, gt_labels=[torch.ones(2, dtype=torch.int64)])
    with pytest.raises(ValueError, match='2\\^20'):
        dt.AnchorGrid([(600, 600)], (4800, 4800), ((32,),))
    with pytest.raises(ValueError, match='exceed the limit of 16'):
        dt.AnchorGrid([(5, 7)], (40, 56), (tuple(range(1, 8)),))
    with pytest.raises(ValueError, match='1 to 8 levels'):
        dt.AnchorGrid([(1, 1)] * 9, (40, 56), ((32,),) * 9)
    lab = torch.zeros(2, 9, dtype=torch.int32)
    with pytest.raises(ValueError, match='ROCm device'):
        dt.sample_balanced(lab, 4, 0.5)
    with pytest.raises(ValueError, match='labels must be torch.int32'):
        dt.sample_balanced(lab.long(), 4, 0.5)
    with pytest.raises(ValueError, match=f'batch_size_per_image must lie in \\[1, {dt.MAX_BATCH}\\]'):
        dt.sample_balanced(lab, dt.MAX_BATCH + 1, 0.5)
    with pytest.raises(ValueError, match='positive_fraction must lie'):
        dt.sample_balanced(lab, 4, 1.5)
    with pytest.raises(ValueError, match=r'keys must be \(2,9\)'):
        dt.sample_balanced(lab, 4, 0.5, keys=torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match='keys must be torch.int32'):
        dt.sample_balanced(lab, 4, 0.5, keys=torch.zeros(2, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match='ROCm device'):
        dt.encode_boxes(f(3, 4), f(3, 4))
    with pytest.raises(ValueError, match=r'reference_boxes must be \(3,4\)'):
        dt.encode_boxes(f(2, 4), f(3, 4))
    with pytest.raises(ValueError, match='four numbers'):
        dt.encode_boxes(f(3, 4), f(3, 4), (1, 1, 1))
    obj, dl = [f(2, 3, 5, 7), f(2, 3, 3, 4)], [f(2, 12, 5, 7), f(2, 12, 3, 4)]
    args = dict(net_sizes=[(37, 53), (40, 50)], padded_size=(40, 56), sizes=((32,), (64,)))
    tg = [_target(), _target(3)]
    with pytest.raises(ValueError, match='ROCm device'):
        dt.rpn_loss(obj, dl, tg, **args)
    with pytest.raises(ValueError, match=r'bbox_deltas\[1\] must be \(2,12,3,4\)'):
        dt.rpn_loss(obj, [dl[0], f(2, 12, 4, 3)], tg, **args)
    with pytest.raises(ValueError, match=r'objectness\[0\] must be contiguous'):
        dt.rpn_loss([f(2, 3, 7, 5).transpose(2, 3), obj[1]], dl, tg, **args)
    with pytest.raises(ValueError, match='3 anchors per cell, sizes x aspect_ratios give 2'):
        dt.rpn_loss(obj, dl, tg, aspect_ratios=(0.5, 1.0), **args)
    with pytest.raises(ValueError, match='one dict per image: 2 images, got 1'):
        dt.rpn_loss(obj, dl, tg[:1], **args)
    with pytest.raises(ValueError, match='holds no ground truth'):
        dt.rpn_loss(obj, dl, [tg[0], _target(0)], **args)
    with pytest.raises(ValueError, match='net_sizes must hold one'):
        dt.rpn_loss(obj, dl, tg, **dict(args, net_sizes=[(37, 53)]))
    with pytest.raises(ValueError, match=r'keys must be \(2,141\)'):
        dt.rpn_loss(obj, dl, tg, keys=torch.zeros(2, 140, dtype=torch.int32), **args)
    cnt = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match='ROCm device'):
        dt.roi_training_samples(f(20, 4), cnt, tg)
    with pytest.raises(ValueError, match='padded rows, the same number'):
        dt.roi_training_samples(f(21, 4), cnt, tg)
    with pytest.raises(ValueError, match=r'counts must be \(2\)'):
        dt.roi_training_samples(f(20, 4), cnt[:1], tg)
    with pytest.raises(ValueError, match=r'keys must be \(2,13\)'):
        dt.roi_training_samples(f(20, 4), cnt, tg, keys=torch.zeros(2, 10, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'targets\[1\] labels must be \(3\)'):
        dt.roi_training_samples(f(20, 4), cnt, [tg[0], dict(tg[1], labels=torch.ones(2, dtype=torch.int64))])
    with pytest.raises(ValueError, match='ROCm device'):
        dt.fastrcnn_loss(f(5, 3), f(5, 12), torch.zeros(5, dtype=torch.int64), f(5, 4))
    with pytest.raises(ValueError, match=r'box_regression must be \(5,12\)'):
        dt.fastrcnn_loss(f(5, 3), f(5, 3), torch.zeros(5, dtype=torch.int64), f(5, 4))
    with pytest.raises(ValueError, match=f'classes lie outside \\[2, {dt.MAX_CLASSES}\\]'):
        dt.fastrcnn_loss(f(5, 1), f(5, 4), torch.zeros(5, dtype=torch.int64), f(5, 4))
    with pytest.raises(ValueError, match=f'classes lie outside \\[2, {dt.MAX_CLASSES}\\]'):
        dt.fastrcnn_loss(f(1, dt.MAX_CLASSES + 1), f(1, 4 * dt.MAX_CLASSES + 4), torch.zeros(1, dtype=torch.int64), f(1, 4))
    with pytest.raises(ValueError, match=r'labels must be \(5\)'):
        dt.fastrcnn_loss(f(5, 3), f(5, 12), torch.zeros(4, dtype=torch.int64), f(5, 4))
    masks = torch.zeros(2, 24, 40, dtype=torch.uint8)
    idx = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match='ROCm device'):
        dt.mask_targets(masks, f(3, 4), idx, 28)
    with pytest.raises(ValueError, match=f'M = {dt.MAX_MASK_SIDE + 1} lies outside'):
        dt.mask_targets(masks, f(3, 4), idx, dt.MAX_MASK_SIDE + 1)
    with pytest.raises(ValueError, match='gt_masks must be torch.uint8'):
        dt.mask_targets(masks.float(), f(3, 4), idx, 28)
    with pytest.raises(ValueError, match=r'matched_idxs must be \(3\)'):
        dt.mask_targets(masks, f(3, 4), idx[:2], 28)
    pos = (f(4, 4), torch.ones(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match='ROCm device'):
        dt.maskrcnn_loss(f(4, 3, 28, 28), *pos, tg)
    with pytest.raises(ValueError, match=r'mask_logits must be \(R,C,M,M\)'):
        dt.maskrcnn_loss(f(4, 3, 28, 14), *pos, tg)
    with pytest.raises(ValueError, match='padded rows, the same number'):
        dt.maskrcnn_loss(f(3, 3, 28, 28), pos[0][:3], pos[1][:3], pos[2][:3], tg)
    with pytest.raises(ValueError, match=r'targets\[0\] masks must be \(2,\*,\*\)'):
        dt.maskrcnn_loss(f(4, 3, 28, 28), *pos, [dict(tg[0], masks=torch.zeros(1, 24, 40, dtype=torch.uint8)), tg[1]])
    with pytest.raises(ValueError, match=r'pos_counts must be \(2\)'):
        dt.maskrcnn_loss(f(4, 3, 28, 28), *pos, tg, pos_counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='ROCm device'):
        dt.detector_losses([f(2, 8, 5, 7), f(2, 8, 3, 4)], lambda x: (obj, dl), None, None, tg, **args)
    # torchvision's training values fit the NMS arena: 2000 x 5 levels <= cosy_nms_max_candidates()
    assert 2000 * 5 <= detector.MAX_CANDIDATES


def test_lazy_names():
    import cosypose_amd
    for name in ('match_boxes', 'sample_balanced', 'encode_boxes', 'rpn_loss', 'roi_training_samples', 'fastrcnn_loss', 'mask_targets',
                 'maskrcnn_loss', 'detector_losses', 'AnchorGrid'):
        assert getattr(cosypose_amd, name) is getattr(dt, name)


def test_abi_names_source_and_flags():
    """the entry points are declared in the header, listed in _lib.EXPORTS and exported by the built library; the source is compiled with
    contraction off"""
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES, FILE_FLAGS
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'cosyhip.h')).read()
    build()
    for name in NAMES:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_dettrain.hip' in SOURCES and '-ffp-contract=off' in FILE_FLAGS['kernels_dettrain.hip']
    for macro, value in (('COSY_DT_MAX_GT', dt.MAX_GT), ('COSY_DT_MAX_BATCH', dt.MAX_BATCH), ('COSY_DT_MAX_CLASSES', dt.MAX_CLASSES),
                         ('COSY_DT_MAX_M', dt.MAX_MASK_SIDE), ('COSY_DT_MAX_GRID', ref.MAX_GRID)):
        assert re.search(rf'#define {macro} {value}\b', header), macro

"""CPU: the twin of the detector's proposal side (tests/detpre_ref.py) against hand-derived vectors, and the
argument checks of cosypose_amd/detector_rpn.py, which must refuse a bad call before the library is even loaded."""
import math

import numpy as np
import pytest
import torch

import detpre_ref as ref
from cosypose_amd import detector, detector_rpn

f32 = np.float32


# ---- the twin against hand-derived vectors ---------------------------------------------------------------------------------------------
def test_twin_base_anchors_of_size_32():
    # ratios 0.5, 1, 2: h_r = sqrt(ratio), w_r = 1 / h_r; 32 (1.41421, 0.70711) / 2 = (22.63, 11.31) -> (23, 11); 16; (11, 23)
    want = [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    assert ref.base_anchors((32,)).tolist() == want
    assert detector_rpn.base_anchors((32,), (0.5, 1.0, 2.0)).tolist() == want
    # half to even: size 2, ratio 1 -> 1; size 1 -> +-0.5 -> 0; size 3 -> 1.5 -> 2; size 5 -> 2.5 -> 2
    assert ref.base_anchors((1, 2, 3, 5), (1.0,))[:, 2].tolist() == [0, 1, 2, 2]
    assert detector_rpn.base_anchors((1, 2, 3, 5), (1.0,))[:, 2].tolist() == [0, 1, 2, 2]


def test_twin_anchor_table_is_the_products_and_in_index_order():
    sizes = [(5, 7), (3, 4), (1, 2)]
    got = ref.anchors(sizes, (40, 56), ((32,), (64,), (128,)))
    assert got.shape == (3 * (35 + 12 + 2), 4)
    assert np.array_equal(got, detector_rpn.rpn_anchors(sizes, (40, 56), ((32,), (64,), (128,))).numpy())
    # level 0, cell (y, x) = (2, 3), a = 1: stride 8 both ways -> [-16, -16, 16, 16] + (24, 16)
    assert got[(2 * 7 + 3) * 3 + 1].tolist() == [8, 0, 40, 32]
    # level 2 (offset 3 (35 + 12)), cell (0, 1), a = 0: stride_w 28; base of size 128, ratio 0.5: (+-91, +-45)
    assert got[3 * 47 + 3].tolist() == [-91 + 28, -45, 91 + 28, 45]
    # a stride that is no integer: 41 / 5 as a float32
    odd = ref.anchors([(5, 7)], (41, 56), ((32,),))
    assert odd[(4 * 7) * 3 + 1, 1] == f32(4) * f32(41 / 5) + f32(-16)


def test_twin_decode_goes_through_the_clamp():
    # anchor 32 x 32 around the origin: dx = 0.5 moves cx to 16, dy = -0.25 moves cy to -8; dw = 5 > log(1000/16): the width is 32 x 62.5 = 2000
    got = ref.decode(np.array([[0.5, -0.25, 5.0, 0.0]], f32), np.array([[-16, -16, 16, 16]], f32)).numpy()[0]
    assert got[1] == -24 and got[3] == 8                                       # exp(0) = 1: exact
    assert abs(got[0] - (16 - 1000)) < 1e-3 and abs(got[2] - (16 + 1000)) < 1e-3
    assert float(got[2] - got[0]) < 32 * math.exp(5) / 2


def test_twin_top_k_takes_equal_logits_lower_index_first():
    d = np.zeros((4, 4), f32)
    assert ref.top_k(np.array([-1, -1, -3, -1], f32), d, 2).tolist() == [0, 1]
    assert ref.top_k(np.array([-1, -1, -3, -1], f32), d, 9).tolist() == [0, 1, 3, 2]
    assert ref.top_k(np.array([-3, 2, -3, 2], f32), d, 3).tolist() == [1, 3, 0]
    assert ref.top_k(np.array([0.0, -0.0, 0.0], f32), d[:3], 2).tolist() == [0, 1]           # -0 counts as +0
    nan_d = d.copy()
    nan_d[1, 2] = np.nan
    assert ref.top_k(np.array([5, 9, np.nan, 1], f32), nan_d, 3).tolist() == [0, 3]      # absent: neither selected nor counted


def test_twin_level_mapper_on_the_canonical_sides():
    """Four levels with k = 3 .. 6.  Sides 111, 223 and 2000 sit farther than 1e-4 from an integer in 4 + log2(s / 224 + 1e-6).  Sides 112, 224
    and 448 CANNOT: s / 224 is a power of two, so the value is an integer plus log2(1 + 1e-6 / (s / 224)) = 2.9e-6, 1.4e-6, 7.2e-7 -- the
    1e-6 of the formula exists to lift exactly these boxes onto the upper level.  They are held to that instead: above the integer by more
    than 5e-7, which float32 resolves at 3 .. 5 (spacing 2.4e-7 .. 4.8e-7) with the sum rounding to the integer or above either way."""
    sides = [111, 112, 223, 224, 448, 2000]
    boxes = np.array([[3, 5, 3 + s, 5 + s] for s in sides], f32)
    off = ref.level_value64(boxes) - np.round(ref.level_value64(boxes))
    print('4 + log2(s / 224 + 1e-6) minus the nearest integer:', dict(zip(sides, off.tolist())))
    assert (np.abs(off[[0, 2, 5]]) > 1e-4).all()
    assert ((off[[1, 3, 4]] > 5e-7) & (off[[1, 3, 4]] < 1e-5)).all()
    assert ref.map_levels(boxes, 3, 6).tolist() == [0, 0, 0, 1, 2, 3]
    assert ref.map_levels(boxes, 2, 5).tolist() == [0, 1, 1, 2, 3, 3]
    # zero area and a negative area (NaN) take level 0; both sides inverted is a positive area
    odd = np.array([[5, 5, 5, 90], [90, 5, 5, 90], [900, 900, 5, 5]], f32)
    assert ref.map_levels(odd, 2, 5).tolist() == [0, 0, 3]


def test_twin_roi_align_hand_values():
    feat = np.array([[[1, 2], [3, 4]]], f32)
    one = lambda box, g=1: float(ref.roi_align(feat, np.array(box, f32), 1.0, 1, g)[0, 0, 0])
    assert one([0, 0, 1, 1]) == 2.5                                            # the sample at (0.5, 0.5): a quarter of each pixel
    assert one([0, 0, 2, 2]) == 4.0                                            # the sample at (1, 1) = size - 1: the last pixel alone
    assert one([0, 0, 1, 1], g=2) == (1.75 + 2.25 + 2.75 + 3.25) / 4           # samples at 0.25 and 0.75 on both axes of 1 + x + 2 y
    assert one([0, -1.5, 1, -0.5]) == 1.5                                      # y = -1 exactly: still inside, clamped to row 0
    assert one([0, -1.75, 1, -0.75]) == 0.0                                    # y = -1.25: outside
    assert one([0, 1.5, 1, 2.5]) == 3.5                                        # y = 2 = h exactly: still inside, the last row
    assert one([0, 1.75, 1, 2.75]) == 0.0                                      # y = 2.25: outside
    assert one([0.2, 0.3, 0.4, 0.5]) == one([0.2, 0.3, 1.2, 1.3])              # an extent below one pixel is clamped to 1
    assert one([0, 0, 2, 2]) == float(ref.roi_align(feat, np.array([0, 0, 4, 4], f32), 0.5, 1, 1)[0, 0, 0])      # the spatial scale
    v64, mag = ref.roi_align(feat, np.array([0, 0, 1, 1], f32), 1.0, 1, 2, np.float64)
    assert float(v64[0, 0, 0]) == 2.5 and float(mag[0, 0, 0]) == 2.5
    assert one([np.nan, 0, 1, 1]) == 0.0


def test_twin_scales_follow_the_larger_image():
    sizes = [(200, 272), (100, 136), (50, 68), (25, 34), (13, 17)]
    assert ref.infer_scales(sizes, [(800, 1067), (750, 1000)]) == [2.0 ** -k for k in range(2, 7)]
    assert detector_rpn.infer_scales(sizes, [(800, 1067), (750, 1000)]) == [2.0 ** -k for k in range(2, 7)]


# ---- the wrappers' checks ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(detector._lib, 'lib', boom)


def test_wrappers_refuse_bad_arguments_before_loading_the_library(no_library):
    f = lambda *s: torch.zeros(*s)
    sizes = ((32,), (64,))
    obj, dl = [f(2, 3, 5, 7), f(2, 3, 3, 4)], [f(2, 12, 5, 7), f(2, 12, 3, 4)]
    args = dict(net_sizes=[(37, 53), (40, 50)], padded_size=(40, 56), sizes=sizes)
    prop = detector_rpn.rpn_proposals
    with pytest.raises(ValueError, match='ROCm device'):
        prop(obj, dl, **args)                                                  # host tensors
    with pytest.raises(ValueError, match=r'objectness\[0\] must be \(B,A,H,W\)'):
        prop([f(2, 3, 35)] + obj[1:], dl, **args)                              # rank
    with pytest.raises(ValueError, match=r'bbox_deltas\[1\] must be \(2,12,3,4\)'):
        prop(obj, [dl[0], f(2, 12, 4, 3)], **args)
    with pytest.raises(ValueError, match=r'objectness\[1\] must be torch.float32'):
        prop([obj[0], obj[1].double()], dl, **args)
    with pytest.raises(ValueError, match=r'bbox_deltas\[0\] must be contiguous'):
        prop(obj, [f(2, 12, 7, 5).transpose(2, 3), dl[1]], **args)
    with pytest.raises(ValueError, match='list of one tensor per level'):
        prop(obj[0], dl[0], **args)
    with pytest.raises(ValueError, match='objectness holds 2 levels, bbox_deltas 1'):
        prop(obj, dl[:1], **args)
    with pytest.raises(ValueError, match='sizes must hold one tuple'):
        prop(obj, dl, **dict(args, sizes=((32,),)))
    with pytest.raises(ValueError, match='3 anchors per cell, sizes x aspect_ratios give 2'):
        prop(obj, dl, aspect_ratios=(0.5, 1.0), **args)
    with pytest.raises(ValueError, match='cosy_nms_max_candidates'):
        prop(obj, dl, pre_nms_top_n=detector.MAX_CANDIDATES // 2 + 1, **args)  # pre_nms_top_n L above the cap
    with pytest.raises(ValueError, match='net_sizes must hold one'):
        prop(obj, dl, **dict(args, net_sizes=[(37, 53)]))
    with pytest.raises(ValueError, match='exceed padded_size'):
        prop(obj, dl, **dict(args, net_sizes=[(37, 53), (41, 50)]))
    with pytest.raises(ValueError, match='must be positive'):
        prop(obj, dl, post_nms_top_n=0, **args)
    with pytest.raises(ValueError, match='2\\^20'):
        detector_rpn.rpn_anchors([(600, 600)], (4800, 4800), ((32,),))
    align = detector_rpn.multiscale_roi_align
    feats = [f(2, 8, 16, 20), f(2, 8, 8, 10)]
    net = [(64, 80), (60, 70)]
    boxes, ids = f(5, 4), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match='ROCm device'):
        align(feats, boxes, net, 7, batch_im_id=ids)
    with pytest.raises(ValueError, match='sampling_ratio must be > 0'):
        align(feats, boxes, net, 7, sampling_ratio=0, batch_im_id=ids)
    with pytest.raises(ValueError, match='sampling_ratio must be > 0'):
        align(feats, boxes, net, 7, sampling_ratio=-1, batch_im_id=ids)
    with pytest.raises(ValueError, match='differs from the scale from the widths'):
        align([f(2, 8, 16, 20), f(2, 8, 8, 5)], boxes, net, 7, batch_im_id=ids)             # 8 / 64 against 5 / 80
    with pytest.raises(ValueError, match=r'features\[1\] must be \(2,8,\*,\*\)'):
        align([feats[0], f(2, 9, 8, 10)], boxes, net, 7, batch_im_id=ids)
    with pytest.raises(ValueError, match=r'features\[0\] must be contiguous'):
        align([f(2, 8, 20, 16).transpose(2, 3), feats[1]], boxes, net, 7, batch_im_id=ids)
    with pytest.raises(ValueError, match='boxes must be'):
        align(feats, f(5, 5), net, 7, batch_im_id=ids)
    with pytest.raises(ValueError, match='exactly one of batch_im_id and counts'):
        align(feats, boxes, net, 7)
    with pytest.raises(ValueError, match='exactly one of batch_im_id and counts'):
        align(feats, boxes, net, 7, batch_im_id=ids, counts=[2, 3])
    with pytest.raises(ValueError, match='summing to 5 rows'):
        align(feats, boxes, net, 7, counts=[2, 2])
    with pytest.raises(ValueError, match='batch_im_id must be'):
        align(feats, boxes, net, 7, batch_im_id=ids[:4])
    with pytest.raises(ValueError, match='output_size x sampling_ratio'):
        align(feats, boxes, net, 65, batch_im_id=ids)
    with pytest.raises(ValueError, match='do not index 2 levels'):
        align(feats, boxes, net, 7, batch_im_id=ids, scales=[0.25, 0.03125])
    with pytest.raises(ValueError, match='ROCm device'):
        detector_rpn.detections_from_features(feats, lambda x: (obj, dl), None, None, args['net_sizes'], (40, 56), [(24, 40)] * 2, {1: 'a'}, sizes=sizes)


def test_lazy_names():
    import cosypose_amd
    for name in ('rpn_anchors', 'rpn_proposals', 'multiscale_roi_align', 'detections_from_features'):
        assert getattr(cosypose_amd, name) is getattr(detector_rpn, name)

"""The twin of the RoIAlign backward (tests/detbwd_ref.py) held against an adjoint it does not share a line with and
against hand-computed weights; the wrappers' checks; the ABI.  Runs without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import detbwd_ref as ref
from cosypose_amd import detector, detector_rpn

f32 = np.float32
CASES = ref.make_cases()


def test_cases_sit_away_from_level_boundaries():
    assert all(ref.away_from_level_boundaries(c['boxes']) for c in CASES)
    levels = ref.row_levels(ref.all_boxes(), np.zeros(len(ref.all_boxes()), np.int64), ref.SCALES, ref.B)
    assert set(levels.tolist()) == {0, 1, 2, 3, 4}                               # every level is some box's


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_hand_derived_adjoint_equals_autograd(case):
    """(a) in float64 against (b): the same real number summed in two orders, so equal to 1e-12 of the largest gradient of the level (its
    terms are at most that large in sum: sum |term| is within a small factor of it for these smooth weights)"""
    args = (case['grad_out'], case['boxes'], case['im_ids'], ref.SHAPES, ref.SCALES, case['P'], case['g'], ref.B)
    mine, mag, cnt = ref.roi_align_backward(*args, dtype=np.float64)
    auto = ref.adjoint_by_autograd(*args)
    for a, b, m in zip(mine, auto, mag):
        assert a.shape == b.shape and np.isfinite(a).all()
        assert (np.abs(a - b) <= 1e-12 * np.maximum(m.max(), 1e-300)).all()
    f = ref.roi_align_backward(*args)                                            # the float32 mode agrees to float32 accuracy
    for a, b, m, n in zip(f, mine, mag, cnt):
        assert a.dtype == f32 and (np.abs(a - b) <= 2.0 ** -24 * (n[:, None] + 4) * m).all()


def one_roi(box, shape, g=1, P=1, grad=1.0):
    go = np.full((1, 1, P, P), grad, f32)
    return ref.roi_align_backward(go, np.array([box], f32), np.zeros(1, np.int64), [shape], [1.0], P, g, 1)[0][0, 0]


def test_twin_hand_values():
    # one RoI, P = 1, g = 1 on a 2 x 2 map: the sample at (y, x) = (0.25, 0.75) -> weights (1-ly)(1-lx), (1-ly) lx, ly (1-lx), ly lx
    got = one_roi([0.25, -0.25, 1.25, 0.75], (2, 2))
    assert got.tolist() == [[0.75 * 0.25, 0.75 * 0.75], [0.25 * 0.25, 0.25 * 0.75]]
    assert one_roi([0, 0, 1, 1], (2, 2)).tolist() == [[0.25, 0.25], [0.25, 0.25]]
    # a sample clamped at the last cell (y = x = 1 = size - 1): lo == hi, both weights on one cell, which gets 1
    assert one_roi([0, 0, 2, 2], (2, 2)).tolist() == [[0, 0], [0, 1]]
    assert one_roi([1.5, 1.5, 2.5, 2.5], (2, 2), grad=3.0).tolist() == [[0, 0], [0, 3]]      # (2, 2) = size exactly: still inside
    # a sample at -1.5: nothing; at -1 exactly: inside, clamped to cell 0
    assert not one_roi([0, -2, 1, -1], (2, 2)).any()
    assert one_roi([0, -1.5, 1, -0.5], (2, 2)).tolist() == [[0.5, 0.5], [0, 0]]
    # g = 2: four samples at 0.25 / 0.75 per axis, each a quarter of the gradient
    assert one_roi([0, 0, 1, 1], (2, 2), g=2).tolist() == [[(0.75 + 0.25) ** 2 / 4, (0.25 + 0.75) ** 2 / 4]] * 2
    v, mag, n = ref.roi_align_backward(np.full((1, 1, 1, 1), -2, f32), np.array([[0, 0, 2, 2]], f32), np.zeros(1, np.int64), [(2, 2)], [1.0], 1, 1, 1,
                                       np.float64)
    assert v[0][0, 0].tolist() == [[0, 0], [0, -2]] and mag[0][0, 0].tolist() == [[0, 0], [0, 2]] and n[0][0].tolist() == [[0, 0], [0, 4]]
    assert not one_roi([np.nan, 0, 1, 1], (2, 2)).any()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(detector._lib, 'lib', boom)


def test_wrappers_refuse_bad_arguments_before_loading_the_library(no_library):
    f = lambda *s: torch.zeros(*s, requires_grad=True)
    feats = [f(2, 3, 5, 7), f(2, 3, 3, 4)]
    boxes, ids = torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32)
    ms = lambda *a, **k: detector_rpn.multiscale_roi_align(*a, **{'scales': [0.125, 0.0625], 'batch_im_id': ids, **k})
    with pytest.raises(ValueError, match='ROCm device'):
        ms(feats, boxes, None, 7)                                               # features that require grad: still refused on the host
    with pytest.raises(ValueError, match='sampling_ratio must be > 0'):
        ms(feats, boxes, None, 7, 0)
    with pytest.raises(ValueError, match=r'7 x 19 must lie in \[1, 128\]'):
        ms(feats, boxes, None, 7, 19)
    with pytest.raises(ValueError, match='1 to 8 levels'):
        ms([f(1, 1, 1, 1)] * 9, boxes, None, 7)
    roi = detector_rpn.roi_align
    with pytest.raises(ValueError, match='ROCm device'):
        roi(feats[0], torch.zeros(4, 5), 7)
    with pytest.raises(ValueError, match='ROCm device'):
        roi(feats[0], [torch.zeros(3, 4), torch.zeros(1, 4)], 7, 0.25)
    with pytest.raises(ValueError, match=r'boxes must be \(\*,5\)'):
        roi(feats[0], boxes, 7)
    with pytest.raises(ValueError, match='sampling_ratio must be > 0'):
        roi(feats[0], torch.zeros(4, 5), 7, 1.0, 0)                             # the adaptive grid stays refused
    with pytest.raises(ValueError, match='sampling_ratio must be > 0'):
        roi(feats[0], torch.zeros(4, 5), 7, 1.0, -1)
    with pytest.raises(ValueError, match='one positive number per level'):
        roi(feats[0], torch.zeros(4, 5), 7, 0.0)
    with pytest.raises(ValueError, match='must hold one non-negative number per image'):
        roi(feats[0], [torch.zeros(3, 4)], 7)


def test_the_differentiable_path_is_taken_only_for_features_that_require_grad(monkeypatch):
    """no GPU here: the launch and the device check are replaced, and which of the two routes asked for it is recorded"""
    taken = []
    monkeypatch.setattr(detector, '_on_device', lambda **k: None)
    monkeypatch.setattr(detector_rpn._lib, 'ints_to_device', lambda v, d: torch.as_tensor(np.asarray(v), dtype=torch.int32))
    plain = lambda call, features: (taken.append('plain'), (torch.zeros(call['R'], call['C'], call['P'], call['P']), None))[1]
    monkeypatch.setattr(detector_rpn, '_msroi_forward', plain)

    class Fn:
        @staticmethod
        def apply(call, *features):
            taken.append('autograd')
            return torch.zeros(call['R'], call['C'], call['P'], call['P']), None
    monkeypatch.setattr(detector_rpn, '_MsroiAlignFn', Fn)
    boxes, ids = torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32)
    run = lambda feats: detector_rpn.multiscale_roi_align(feats, boxes, None, 7, scales=[0.125, 0.0625], batch_im_id=ids)
    fixed = [torch.zeros(2, 3, 5, 7), torch.zeros(2, 3, 3, 4)]
    run(fixed)
    run([fixed[0], fixed[1].clone().requires_grad_(True)])
    with torch.no_grad():
        run([t.clone().requires_grad_(True) for t in fixed])
    run([t.clone().requires_grad_(True) for t in fixed])
    assert taken == ['plain', 'autograd', 'plain', 'autograd']


def test_lazy_names():
    import cosypose_amd
    assert cosypose_amd.roi_align is detector_rpn.roi_align and cosypose_amd.multiscale_roi_align is detector_rpn.multiscale_roi_align


def test_abi_names_source_and_flags():
    """the entry point is declared in the header, listed in _lib.EXPORTS with as many arguments as the header names, and exported by the
    built library; its source file is compiled with contraction off"""
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES, FILE_FLAGS
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'cosyhip.h')).read()
    build()
    name = 'cosy_msroi_align_backward'
    decl = re.search(r'\bint ' + name + r'\s*\(([^;]*)\);', header)
    assert decl and name in _lib.EXPORTS           # test_c_abi.py: the library exports what EXPORTS names
    assert len(decl.group(1).split(',')) == len(_lib._SIGNATURES[name][0]) == 17
    src = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'kernels_detpre.hip')).read()
    assert re.search(r'\bint ' + name + r'\s*\(', src) and 'kernels_detpre.hip' in SOURCES and '-ffp-contract=off' in FILE_FLAGS['kernels_detpre.hip']
    assert '#pragma clang fp contract(off)' in src
    assert detector_rpn.MAX_LEVELS == _lib.RPN_MAX_LEVELS == int(re.search(r'#define COSY_RPN_MAX_LEVELS (\d+)', header).group(1))

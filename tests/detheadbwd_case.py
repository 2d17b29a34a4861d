"""The cases that tests/test_detector_heads_backward_host.py (CPU) and tests/test_detector_heads_backward.py (GPU) share: the single-layer shapes
of tests/dethead_case.py (imported, not copied: both row tiles, one and four channel tiles, partial k-blocks, C_in 8 and 40, C_out 3 / 15 / 24 /
88, M = 0, 1, 5, 65, 257, 1025, the 1 x 2 map that is all border, the 14 x 14 deconvolution), each with a seeded upstream gradient; four tiny
linear layers whose row counts sit on the edges of the weight gradient's slab; and dethead_case's whole-head weights and inputs with seeded
gradients at the heads' raw outputs.  The twin's references are computed once per process and handed out unchanged.

SALT was picked on the CPU (the first value from 1 up) so that frames_ref.fma32's DoubleRounding guard fires on no case, single layers and whole
heads alike: tests/test_detector_heads_backward_host.py runs them all and would raise."""
import functools

import numpy as np

import dethead_case as fc
import dethead_ref as ref
import detheadbwd_ref as bref

F32 = np.float32
SLAB = 256                               # cells of a weight-gradient slab below 16 slabs: the GPU tests hold the library to it
SLAB_CASES = [('linear', 8, 3, False, M, 1, 1) for M in (SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3)]
CASES = list(fc.CASES) + SLAB_CASES
SALT = 1
case_id = fc.case_id


def out_shape(case):
    kind, ci, co, relu, B, H, W = case
    return (B, co) if kind == 'linear' else (B, co, 2 * H, 2 * W) if kind == 'deconv' else (B, co, H, W)


@functools.lru_cache(maxsize=None)
def case_grad(case):
    """the seeded gradient at the layer's pre-activation output, float32"""
    rng = np.random.RandomState(7919 * SALT + sum(ord(c) * (i + 3) for i, c in enumerate(case_id(case))))
    return rng.normal(0, 1, out_shape(case)).astype(F32)


@functools.lru_cache(maxsize=None)
def want(case):
    """-> dict(dx32, dx64, dW, db, S_W, S_b, T_W, T_b) of the twin (dx32 raises DoubleRounding where the emulation is unsafe)"""
    layer, x = fc.case_data(case)
    g = case_grad(case)
    out = bref.wgrad64(layer, x, g)
    out.update(dx32=bref.dx32(layer, g), dx64=bref.dx64(layer, g))
    return out


# ---- whole heads ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_grads(seed=17):
    """gradients at the raw outputs: rpn [per level (B, 5A, H, W): objectness columns first], box (R, 5K), mask (D, K, 28, 28)"""
    rng = np.random.RandomState(seed + SALT)
    bits = fc.head_bits()
    return dict(rpn=[rng.normal(0, 1, o.shape).astype(F32) for o in bits['rpn']], box=rng.normal(0, 1, bits['box'].shape).astype(F32),
                mask=rng.normal(0, 1, bits['mask'].shape).astype(F32))


def split(d, n):
    """one wgrad64 dict of a sibling GEMM -> the two layers' dicts (outputs [0, n) and the rest)"""
    cut = lambda v, a, b: v[a:b] if isinstance(v, np.ndarray) else v
    return ({k: cut(v, 0, n) for k, v in d.items()}, {k: cut(v, n, None) for k, v in d.items()})


def add(a, b):
    """the sum over two groups of cells (the RPN's levels, each a chain of its own in the twin): values and measures add, T too"""
    return {k: a[k] + b[k] for k in a}


@functools.lru_cache(maxsize=None)
def head_wants():
    """-> dict(rpn=(dX per level, {param name: wgrad dict}), box=..., mask=...): the twin's chained backward of the three heads"""
    sd, (feats, roi, mroi), g = fc.head_weights(), fc.head_inputs(), head_grads()
    out = {}
    per_level = [bref.head_backward(ref.rpn_layers(sd), f, gl) for f, gl in zip(feats, g['rpn'])]
    conv, pred = per_level[0][1]
    for _, (c, p) in per_level[1:]:
        conv, pred = add(conv, c), add(pred, p)
    cls, box = split(pred, fc.A)
    out['rpn'] = ([dx for dx, _ in per_level], {'rpn.head.conv': conv, 'rpn.head.cls_logits': cls, 'rpn.head.bbox_pred': box})
    dx, (fc6, fc7, pred) = bref.head_backward(ref.box_layers(sd), roi.reshape(len(roi), -1), g['box'])
    cls, box = split(pred, fc.K)
    out['box'] = (dx.reshape(roi.shape), {'roi_heads.box_head.fc6': fc6, 'roi_heads.box_head.fc7': fc7, 'roi_heads.box_predictor.cls_score': cls,
                                          'roi_heads.box_predictor.bbox_pred': box})
    dx, grads = bref.head_backward(ref.mask_layers(sd), mroi, g['mask'])
    names = [f'roi_heads.mask_head.mask_fcn{i}' for i in range(1, 5)] + ['roi_heads.mask_predictor.conv5_mask', 'roi_heads.mask_predictor.mask_fcn_logits']
    out['mask'] = (dx, dict(zip(names, grads)))
    return out

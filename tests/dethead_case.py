"""The cases that tests/test_detector_heads_host.py (CPU) and tests/test_detector_heads.py (GPU) share: seeded layers of the detector's heads
at the smallest shapes at which cosy_head_conv takes each of its paths, and one seeded set of head weights under torchvision's names.
The twin's references are computed once per process and handed out unchanged."""
import functools

import numpy as np

import dethead_ref as ref

F32 = np.float32
DTYPES = ('float32', 'float16', 'bfloat16')
BIG_ROWS, TILE_ROWS = 1024, 256          # the launcher's threshold and its largest row tile: the GPU tests hold the library to these

# (kind, C_in, C_out, relu, B, H, W): 3x3 convs.  C_in = 40: one full 32-deep k-block and a partial one (float32: two full 16-deep and a
# partial one); 8: less than one.  (1,2): every tap but the centre row is a border.
CONV3 = [('conv3', ci, co, co == 24, 2, H, W) for ci in (40, 8) for co in (3, 15, 24) for H, W in ((5, 7), (3, 4), (1, 2))]
# 1025 rows = 4 tiles of 256 + 1: the large row tile with one channel tile per wave (24 -> 2 tiles) and with four (88 -> 6 tiles: the second
# group of four holds two); the small row tile with four channel tiles; a 1x1 conv
PATHS = [('conv3', 8, 24, True, 1, 25, 41), ('conv3', 40, 88, False, 1, 25, 41), ('conv1', 40, 88, True, 2, 5, 7), ('conv1', 40, 15, False, 2, 5, 7)]
# linear layers, K = 392 = 8 x 49; M = 0, 1, 5, one more than the small tile, one more than a multiple of it below the threshold, and one
# more than a multiple of the large tile
LINEAR = [('linear', 392, co, co == 24, M, 1, 1) for co, Ms in ((24, (0, 1, 5, 65, 257, 1025)), (15, (5, 1025))) for M in Ms]
DECONV = [('deconv', 16, 8, True, 3, 14, 14)]
CASES = CONV3 + PATHS + LINEAR + DECONV
SALT = 1                                 # chosen so that frames_ref.fma32's DoubleRounding guard fires on no case (test_detector_heads_host.py)


def case_id(case):
    return '-'.join(str(int(v)) if not isinstance(v, str) else v for v in case)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> twin layer dict (float32 weights), input x (float32): NCHW, or (M, K) for a linear layer"""
    kind, ci, co, relu, B, H, W = case
    rng = np.random.RandomState(SALT + sum(ord(c) * (i + 1) for i, c in enumerate(case_id(case))))     # a seed of the case's own, the same in every process
    if kind == 'linear':
        w, x = rng.normal(0, 1, (co, ci)) / np.sqrt(ci), rng.normal(0, 1, (B, ci))
    elif kind == 'deconv':
        w, x = rng.normal(0, 1, (ci, co, 2, 2)) / np.sqrt(ci), rng.normal(0, 1, (B, ci, H, W))
    else:
        k = 3 if kind == 'conv3' else 1
        w, x = rng.normal(0, 1, (co, ci, k, k)) / np.sqrt(ci * k * k), rng.normal(0, 1, (B, ci, H, W))
    layer = dict(kind='conv' if kind.startswith('conv') else kind, weight=w.astype(F32), bias=rng.normal(0, 0.5, co).astype(F32), relu=bool(relu))
    return layer, x.astype(F32)


@functools.lru_cache(maxsize=None)
def want64(case, dtype):
    """-> value, bound (K + 2) u S of the twin's float64 evaluation fed the operands rounded to dtype"""
    layer, x = case_data(case)
    v, S, K = ref.layer64(layer, x, dtype)
    return v, (K + 2) * ref.U[dtype] * S


@functools.lru_cache(maxsize=None)
def want32(case):
    """the float32 fmaf chain (raises DoubleRounding where the emulation is unsafe)"""
    return ref.layer32(*case_data(case))


# ---- whole heads: RPN C = 16, A = 3; box head C = 8 (x 49 = 392), hidden 24, K = 3 classes; mask head C = 16, K = 3 ---------------------
RPN_C, A, BOX_C, HIDDEN, K, MASK_C = 16, 3, 8, 24, 3, 16
RPN_GRID = [(5, 7), (3, 4), (1, 2)]


@functools.lru_cache(maxsize=None)
def head_weights(seed=3):
    """{name: float32 array} under torchvision 0.4.2's Mask R-CNN keys, with a few trunk / FPN keys that the loader must ignore"""
    rng = np.random.RandomState(seed)
    sd = {}

    def put(name, shape, fan_in):
        sd[name + '.weight'] = (rng.normal(0, 1, shape) / np.sqrt(fan_in)).astype(F32)
        sd[name + '.bias'] = rng.normal(0, 0.3, shape[1] if 'conv5_mask' in name else shape[0]).astype(F32)
    sd['backbone.body.conv1.weight'] = rng.normal(0, 1, (4, 3, 7, 7)).astype(F32)
    sd['backbone.fpn.inner_blocks.0.weight'] = rng.normal(0, 1, (4, 4, 1, 1)).astype(F32)
    put('rpn.head.conv', (RPN_C, RPN_C, 3, 3), RPN_C * 9)
    put('rpn.head.cls_logits', (A, RPN_C, 1, 1), RPN_C)
    put('rpn.head.bbox_pred', (4 * A, RPN_C, 1, 1), RPN_C)
    put('roi_heads.box_head.fc6', (HIDDEN, BOX_C * 49), BOX_C * 49)
    put('roi_heads.box_head.fc7', (HIDDEN, HIDDEN), HIDDEN)
    put('roi_heads.box_predictor.cls_score', (K, HIDDEN), HIDDEN)
    put('roi_heads.box_predictor.bbox_pred', (4 * K, HIDDEN), HIDDEN)
    for i in range(1, 5):
        put(f'roi_heads.mask_head.mask_fcn{i}', (MASK_C, MASK_C, 3, 3), MASK_C * 9 / 2)
    put('roi_heads.mask_predictor.conv5_mask', (MASK_C, MASK_C, 2, 2), MASK_C / 2)
    put('roi_heads.mask_predictor.mask_fcn_logits', (K, MASK_C, 1, 1), MASK_C)
    return sd


@functools.lru_cache(maxsize=None)
def head_inputs(seed=5):
    """-> RPN features (three levels, B = 2), box RoI features (6 rows, the last all zero: a padding row), mask RoI features (3 rows)"""
    rng = np.random.RandomState(seed)
    feats = [rng.normal(0, 1, (2, RPN_C, H, W)).astype(F32) for H, W in RPN_GRID]
    roi = rng.normal(0, 1, (6, BOX_C, 7, 7)).astype(F32)
    roi[5] = 0
    return feats, roi, rng.normal(0, 1, (3, MASK_C, 14, 14)).astype(F32)


@functools.lru_cache(maxsize=None)
def head_wants(dtype):
    """the twin's chained values and running bounds of the three heads on head_inputs()"""
    sd, (feats, roi, mroi) = head_weights(), head_inputs()
    return dict(rpn=ref.rpn_head(sd, feats, dtype), box=ref.box_head(sd, roi, dtype), mask=ref.mask_head(sd, mroi, dtype))


@functools.lru_cache(maxsize=None)
def head_bits():
    """the float32 heads as chains of the twin's fmaf chains: rpn [per level (B, 5A, H, W)], box (R, 5K), mask (D, K, 28, 28)"""
    sd, (feats, roi, mroi) = head_weights(), head_inputs()
    return dict(rpn=[ref.chain32(ref.rpn_layers(sd), f) for f in feats], box=ref.chain32(ref.box_layers(sd), roi.reshape(len(roi), -1)),
                mask=ref.chain32(ref.mask_layers(sd), mroi))


# ---- the same heads as plain torch.nn modules with torchvision's attribute names -----------------------------------------------------------
def torch_heads(sd=None, dtype=None, device='cpu'):
    """-> rpn_head, box_head, box_predictor, mask_head, mask_predictor modules holding head_weights() (eval, no grad)"""
    import torch
    from torch import nn
    sd = head_weights() if sd is None else sd
    dtype = torch.float32 if dtype is None else dtype
    RPN_C, A = sd['rpn.head.conv.weight'].shape[0], sd['rpn.head.cls_logits.weight'].shape[0]            # the widths are the weights' own
    HIDDEN, BOX_C, K = sd['roi_heads.box_head.fc6.weight'].shape[0], sd['roi_heads.box_head.fc6.weight'].shape[1] // 49, sd['roi_heads.box_predictor.cls_score.weight'].shape[0]
    MASK_C = sd['roi_heads.mask_head.mask_fcn1.weight'].shape[0]

    class RPNHead(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.cls_logits, self.bbox_pred = nn.Conv2d(RPN_C, RPN_C, 3, padding=1), nn.Conv2d(RPN_C, A, 1), nn.Conv2d(RPN_C, 4 * A, 1)

        def forward(self, feats):
            hidden = [torch.relu(self.conv(f)) for f in feats]
            return [self.cls_logits(h) for h in hidden], [self.bbox_pred(h) for h in hidden]

    class TwoMLPHead(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc6, self.fc7 = nn.Linear(BOX_C * 49, HIDDEN), nn.Linear(HIDDEN, HIDDEN)

        def forward(self, x):
            return torch.relu(self.fc7(torch.relu(self.fc6(x.flatten(1)))))

    class FastRCNNPredictor(nn.Module):
        def __init__(self):
            super().__init__()
            self.cls_score, self.bbox_pred = nn.Linear(HIDDEN, K), nn.Linear(HIDDEN, 4 * K)

        def forward(self, x):
            return self.cls_score(x), self.bbox_pred(x)

    class MaskRCNNHeads(nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(1, 5):
                setattr(self, f'mask_fcn{i}', nn.Conv2d(MASK_C, MASK_C, 3, padding=1))

        def forward(self, x):
            for i in range(1, 5):
                x = torch.relu(getattr(self, f'mask_fcn{i}')(x))
            return x

    class MaskRCNNPredictor(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv5_mask, self.mask_fcn_logits = nn.ConvTranspose2d(MASK_C, MASK_C, 2, 2), nn.Conv2d(MASK_C, K, 1)

        def forward(self, x):
            return self.mask_fcn_logits(torch.relu(self.conv5_mask(x)))

    mods = dict(zip(('rpn.head', 'roi_heads.box_head', 'roi_heads.box_predictor', 'roi_heads.mask_head', 'roi_heads.mask_predictor'),
                    (RPNHead(), TwoMLPHead(), FastRCNNPredictor(), MaskRCNNHeads(), MaskRCNNPredictor())))
    for prefix, m in mods.items():
        m.load_state_dict({k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix + '.')})
        m.to(device=device, dtype=dtype).eval().requires_grad_(False)
    return tuple(mods.values())


# ---- features -> detections: one channel count for the three heads ------------------------------------------------------------------------
CHAIN_C = 8


@functools.lru_cache(maxsize=None)
def chain_weights(seed=11):
    """head weights over CHAIN_C-channel features for detections_from_features.  The RPN's SIZE deltas are zero: exp(0) = 1 on the device and in
    the twin, so the proposals are bit-equal on both sides and everything behind them sees the same inputs (tests/test_detector_rpn.py's
    device); the class weights are spread so that both classes are found"""
    rng = np.random.RandomState(seed)
    C, sd = CHAIN_C, {}

    def put(name, shape, scale, bias=0.1):
        sd[name + '.weight'] = (rng.normal(0, 1, shape) * scale).astype(F32)
        sd[name + '.bias'] = (rng.normal(0, 1, shape[1] if 'conv5_mask' in name else shape[0]) * bias).astype(F32)
    put('rpn.head.conv', (C, C, 3, 3), 0.3)
    put('rpn.head.cls_logits', (A, C, 1, 1), 0.3)
    put('rpn.head.bbox_pred', (4 * A, C, 1, 1), 0.3)
    sd['rpn.head.bbox_pred.weight'].reshape(A, 4, C)[:, 2:] = 0
    sd['rpn.head.bbox_pred.bias'].reshape(A, 4)[:, 2:] = 0
    put('roi_heads.box_head.fc6', (16, C * 49), 0.3 / 7)
    put('roi_heads.box_head.fc7', (16, 16), 0.3)
    put('roi_heads.box_predictor.cls_score', (K, 16), 2.4)
    put('roi_heads.box_predictor.bbox_pred', (4 * K, 16), 0.06)
    for i in range(1, 5):
        put(f'roi_heads.mask_head.mask_fcn{i}', (C, C, 3, 3), 0.3)
    put('roi_heads.mask_predictor.conv5_mask', (C, C, 2, 2), 0.5)
    put('roi_heads.mask_predictor.mask_fcn_logits', (K, C, 1, 1), 1.0)
    return sd


def chain_twin_heads(sd):
    """the three heads as the twin's float32 fmaf chains, numpy in, numpy out, with the signatures detpre_ref.chain calls"""
    def rpn(feats):
        out = [ref.chain32(ref.rpn_layers(sd), f) for f in feats]
        return [o[:, :A] for o in out], [o[:, A:] for o in out]

    def box(roi):
        out = ref.chain32(ref.box_layers(sd), np.asarray(roi, F32).reshape(len(roi), -1))
        return out[:, :K], out[:, K:]

    def mask(roi):
        return ref.chain32(ref.mask_layers(sd), np.asarray(roi, F32))
    return rpn, box, mask

"""The detector's heads on the matrix pipe: Mask R-CNN's RPN head, box head + predictor and mask head + predictor (torchvision 0.4.2), the
convolutions and linears between the FPN and detector.detections_from_heads.  Inference only: training keeps the torch modules and autograd
(detector_train.detector_losses).  DESIGN.md section 26 states the contract; HIP: csrc/kernels_dethead.hip (cosy_head_pack, cosy_head_conv).

Every layer is one implicit GEMM over ROWS: a row is one cell (level, image, y, x) with its channels contiguous in the storage type (float32,
float16 or bfloat16; a linear layer's row is its input vector).  The heads' inputs arrive as contiguous NCHW float32 (what the FPN and
multiscale_roi_align produce) and are packed into rows once; the heads' outputs leave as NCHW float32 (what rpn_proposals and
detections_from_heads read in place); between the layers of a head the rows stay in the storage type.  Sibling layers (the RPN's cls_logits /
bbox_pred, the box predictor's cls_score / bbox_pred) run as ONE GEMM whose columns are split on the store.  Weights are packed once, at
construction.  Launches: rpn_head = one pack per level + 2 GEMMs over all levels; box_head = (one cast for the 16-bit types +) 3 GEMMs;
mask_head = one pack + 6 GEMMs.
"""
import ctypes

import torch

from . import _lib

MAX_LEVELS = _lib.RPN_MAX_LEVELS
MAX_ROWS = 1 << 30
_DTYPES = _lib.DTYPES

RPN_KEYS = ('rpn.head.conv', 'rpn.head.cls_logits', 'rpn.head.bbox_pred')
BOX_KEYS = ('roi_heads.box_head.fc6', 'roi_heads.box_head.fc7', 'roi_heads.box_predictor.cls_score', 'roi_heads.box_predictor.bbox_pred')
MASK_KEYS = tuple(f'roi_heads.mask_head.mask_fcn{i}' for i in range(1, 5)) + ('roi_heads.mask_predictor.conv5_mask',
                                                                             'roi_heads.mask_predictor.mask_fcn_logits')


def _dtype(dtype):
    if dtype not in _DTYPES:
        raise ValueError(f'dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype}')
    return dtype


def pack_weight(w, dtype):
    """(N, taps, C_in) float32 CPU -> the fragment order cosy_head_conv reads (cosyhip.h): [N_pad / 16][tap][k-block][lane][element], zero padded"""
    N, taps, C = (int(v) for v in w.shape)
    KB = 16 if dtype == torch.float32 else 32
    KBn, NP = -(-C // KB), -(-N // 64) * 64
    wp = torch.zeros((NP, taps, KBn * KB), dtype=torch.float32)
    wp[:N, :, :C] = w
    E = KB // 4                          # elements of a lane: channel k = E g + e of the block, g = lane >> 4
    wp = wp.view(NP // 16, 16, taps, KBn, 4, E).permute(0, 2, 3, 4, 1, 5)          # nt, i, tap, kb, g, e -> nt, tap, kb, g, i, e
    return wp.contiguous().to(dtype).reshape(-1)


class HeadLayer:
    """one packed layer: kind 'conv' (ksize 3 or 1), 'linear' or 'deconv'; c_in channels of a row, c_out columns of the GEMM, n_out channels of
    the result (deconv: c_out / 4).  w, bias: device tensors in the kernel's order; packed: the same on the CPU (tests compare bytes)"""

    def __init__(self, kind, weight, bias, ksize, relu, dtype, device):
        self.kind, self.ksize, self.relu, self.dtype = kind, int(ksize), bool(relu), _dtype(dtype)
        N, taps, C = (int(v) for v in weight.shape)
        if C < 8 or C % 8:
            raise ValueError(f'{kind} layer: the reduction length {C} must be a positive multiple of 8 (it is not padded silently)')
        self.c_in, self.c_out = C, N
        self.n_out = N // 4 if kind == 'deconv' else N
        self.packed = pack_weight(weight, dtype)
        b = torch.zeros(-(-N // 64) * 64, dtype=torch.float32)
        b[:N] = bias
        self.packed_bias = b
        self.device = torch.device(device) if device is not None else None
        self.w = self.packed.to(self.device) if self.device is not None else None
        self.bias = b.to(self.device) if self.device is not None else None

    @staticmethod
    def _f32(t, name, dims):
        if not torch.is_tensor(t) or t.dim() != dims:
            raise ValueError(f'{name} must be a {dims}-d tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
        return t.detach().to(device='cpu', dtype=torch.float32)

    @staticmethod
    def _bias(bias, n, name):
        if bias is None:
            return torch.zeros(n, dtype=torch.float32)
        b = HeadLayer._f32(bias, name, 1)
        if b.shape[0] != n:
            raise ValueError(f'{name} must be ({n}), got {tuple(b.shape)}')
        return b

    @classmethod
    def conv(cls, weight, bias=None, relu=False, dtype=torch.float32, device=None):
        """Conv2d weight (C_out, C_in, k, k) with k = 3 (pad 1, stride 1) or 1"""
        w = cls._f32(weight, 'weight', 4)
        k = int(w.shape[2])
        if k not in (1, 3) or w.shape[3] != k:
            raise ValueError(f'a conv layer is 3x3 or 1x1, got a kernel of {tuple(w.shape[2:])}')
        return cls('conv', w.permute(0, 2, 3, 1).reshape(w.shape[0], k * k, w.shape[1]), cls._bias(bias, w.shape[0], 'bias'), k, relu, dtype, device)

    @classmethod
    def linear(cls, weight, bias=None, relu=False, dtype=torch.float32, device=None):
        """Linear weight (N, K)"""
        w = cls._f32(weight, 'weight', 2)
        return cls('linear', w.reshape(w.shape[0], 1, w.shape[1]), cls._bias(bias, w.shape[0], 'bias'), 1, relu, dtype, device)

    @classmethod
    def deconv(cls, weight, bias=None, relu=False, dtype=torch.float32, device=None):
        """ConvTranspose2d(k=2, s=2, pad 0) weight (C_in, C_out, 2, 2): a GEMM to the 4 C_out columns (o, dy, dx)"""
        w = cls._f32(weight, 'weight', 4)
        if tuple(w.shape[2:]) != (2, 2):
            raise ValueError(f'a deconv layer is ConvTranspose2d(k=2, s=2), got a kernel of {tuple(w.shape[2:])}')
        Co = int(w.shape[1])
        return cls('deconv', w.reshape(w.shape[0], 4 * Co).t().reshape(4 * Co, 1, w.shape[0]), cls._bias(bias, Co, 'bias').repeat_interleave(4), 1, relu,
                   dtype, device)

    @classmethod
    def siblings(cls, first, second, kind, dtype=torch.float32, device=None):
        """two layers over the same input, (weight, bias) each, as one GEMM: the columns of `first`, then those of `second`"""
        make = cls.conv if kind == 'conv' else cls.linear
        dims = 4 if kind == 'conv' else 2
        w = torch.cat([cls._f32(first[0], 'weight', dims), cls._f32(second[0], 'weight', dims)])
        b = torch.cat([cls._bias(first[1], first[0].shape[0], 'bias'), cls._bias(second[1], second[0].shape[0], 'bias')])
        layer = make(w, b, False, dtype, device)
        layer.n_split = int(first[0].shape[0])
        return layer


# ---- launches ------------------------------------------------------------------------------------------------------------------------
def _check_input(x, name, dims, channels, what):
    """the style of detector_rpn: a ValueError that names the argument, before anything touches the library"""
    if not torch.is_tensor(x):
        raise ValueError(f'{name} must be a tensor, got {type(x).__name__}')
    if x.dim() != dims:
        raise ValueError(f'{name} must be {what}, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise ValueError(f'{name} must be torch.float32, got {x.dtype}')
    if int(x.shape[1]) != channels:
        raise ValueError(f'{name} must be {what} with {channels} channels (the packed weights), got {tuple(x.shape)}')
    return x


def _on_device(x, name):
    """after every shape and dtype check, before anything touches the library"""
    if not x.is_cuda:
        raise ValueError(f'{name} must live on the ROCm device (got a CPU tensor); there is no CPU fallback')
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError(f'{name} requires grad: DetectorHeads is inference only, training keeps the torch.nn modules and autograd '
                           '(detector_train.detector_losses); call it under torch.no_grad() or detach the input')
    return x.contiguous()


def _ready(layer, dev):
    """the layer's weights on the input's device: a layer packed without a device is uploaded on its first use and stays there; a layer
    that lives on another device is refused (a silent re-upload would move the weights under another stream's feet)"""
    if layer.w is None:
        layer.w, layer.bias, layer.device = layer.packed.to(dev), layer.packed_bias.to(dev), dev
    elif layer.w.device != dev:
        raise ValueError(f'the input lives on {dev}, the packed weights on {layer.w.device}: build the heads with device={dev!s}')
    return layer


def _rows(n, c, layer, dev):
    return torch.empty((n, c), dtype=layer.dtype, device=dev)


def _pack(x, rows, B, C, HW, dtype):
    """contiguous NCHW float32 -> rows of the storage type (one launch)"""
    if B:
        _lib.check(_lib.lib().cosy_head_pack(_lib.ptr(x), rows.data_ptr(), B, C, HW, _DTYPES[dtype], _lib.stream()))


def _gemm(layer, x_rows, maps, store, out, out1=None, n_split=None):
    """one launch of layer over x_rows; maps: [(images, H, W)] per level, in row order"""
    d = _lib.HeadLayer()
    d.x, d.w, d.bias, d.out, d.out1 = _lib.ptr(x_rows), _lib.ptr(layer.w), _lib.ptr(layer.bias), _lib.ptr(out), _lib.ptr(out1)
    d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store = _DTYPES[layer.dtype], layer.ksize, layer.c_in, layer.c_out, int(layer.relu), store
    d.n_split = layer.c_out if n_split is None else n_split
    d.n_levels = len(maps)
    row = 0
    for l, (n, H, W) in enumerate(maps):
        d.row_start[l], d.H[l], d.W[l] = row, H, W
        row += n * H * W
        if row > MAX_ROWS:
            raise ValueError(f'{row} rows (cells of all maps) exceed the limit of 2^30 per launch')
    d.row_start[len(maps)] = row
    if row:
        _lib.check(_lib.lib().cosy_head_conv(ctypes.byref(d), _lib.stream()))
    return out


def conv_layer(x, layer):
    """One layer through the kernel.  conv: x (B,C,H,W) -> (B,N,H,W); linear: x (M,K) -> (M,N); deconv: x (B,C,H,W) -> (B,N/4,2H,2W).
    x float32, contiguous, on the device; the result is float32 NCHW.  x is rounded to the layer's storage type on the way in."""
    if not isinstance(layer, HeadLayer):
        raise ValueError(f'layer must be a HeadLayer, got {type(layer).__name__}')
    if layer.kind == 'linear':
        x = _on_device(_check_input(x, 'x', 2, layer.c_in, '(M,K)'), 'x')
        dev = x.device
        _ready(layer, dev)
        M = int(x.shape[0])
        rows = x
        if layer.dtype != torch.float32:
            rows = _rows(M, layer.c_in, layer, dev)
            _pack(x, rows, M, layer.c_in, 1, layer.dtype)
        return _gemm(layer, rows, [(M, 1, 1)], _lib.HEAD_STORE_NCHW, torch.empty((M, layer.c_out), dtype=torch.float32, device=dev))
    x = _on_device(_check_input(x, 'x', 4, layer.c_in, '(B,C,H,W)'), 'x')
    dev = x.device
    _ready(layer, dev)
    B, C, H, W = (int(v) for v in x.shape)
    if B and H * W < 1:
        raise ValueError(f'x must have at least one cell, got {tuple(x.shape)}')
    rows = _rows(B * H * W, C, layer, dev)
    _pack(x, rows, B, C, H * W, layer.dtype)
    if layer.kind == 'deconv':
        return _gemm(layer, rows, [(B, H, W)], _lib.HEAD_STORE_DECONV_NCHW, torch.empty((B, layer.n_out, 2 * H, 2 * W), dtype=torch.float32, device=dev))
    return _gemm(layer, rows, [(B, H, W)], _lib.HEAD_STORE_NCHW, torch.empty((B, layer.c_out, H, W), dtype=torch.float32, device=dev))


# ---- the three heads -----------------------------------------------------------------------------------------------------------------
class RpnHead:
    """rpn_head(features) -> (objectness, bbox_deltas): per level (B,A,H,W) and (B,4A,H,W) float32, views of two flat buffers"""

    def __init__(self, conv, pred):
        self.conv, self.pred = conv, pred
        self.A = pred.n_split
        if pred.c_out != 5 * self.A:
            raise ValueError(f'rpn.head.bbox_pred must have 4 x the {self.A} outputs of cls_logits, got {pred.c_out - self.A}')

    def __call__(self, features):
        if torch.is_tensor(features) or not isinstance(features, (list, tuple)):
            raise ValueError(f'features must be a list of one tensor per level, got {type(features).__name__}')
        if not 1 <= len(features) <= MAX_LEVELS:
            raise ValueError(f'features must hold 1 to {MAX_LEVELS} levels, got {len(features)}')
        feats = [_check_input(f, f'features[{l}]', 4, self.conv.c_in, '(B,C,H,W)') for l, f in enumerate(features)]
        B = int(feats[0].shape[0])
        if any(int(f.shape[0]) != B for f in feats):
            raise ValueError(f'every level must hold the same {B} images, got {[tuple(f.shape) for f in feats]}')
        if B and any(f.shape[2] < 1 or f.shape[3] < 1 for f in feats):
            raise ValueError(f'features must have at least one cell, got {[tuple(f.shape) for f in feats]}')
        feats = [_on_device(f, f'features[{l}]') for l, f in enumerate(feats)]
        dev = feats[0].device
        _ready(self.conv, dev), _ready(self.pred, dev)
        maps = [(B, int(f.shape[2]), int(f.shape[3])) for f in feats]
        starts = [0]
        for n, H, W in maps:
            starts.append(starts[-1] + n * H * W)
        M, C, A = starts[-1], self.conv.c_in, self.A
        x = _rows(M, C, self.conv, dev)
        for l, f in enumerate(feats):
            _pack(f, x[starts[l]:starts[l + 1]], B, C, maps[l][1] * maps[l][2], self.conv.dtype)
        hidden = _gemm(self.conv, x, maps, _lib.HEAD_STORE_ROWS, _rows(M, self.conv.c_out, self.conv, dev))
        obj = torch.empty(A * M, dtype=torch.float32, device=dev)
        dlt = torch.empty(4 * A * M, dtype=torch.float32, device=dev)
        _gemm(self.pred, hidden, maps, _lib.HEAD_STORE_NCHW, obj, dlt, n_split=A)
        return ([obj[A * starts[l]:A * starts[l + 1]].view(B, A, H, W) for l, (_, H, W) in enumerate(maps)],
                [dlt[4 * A * starts[l]:4 * A * starts[l + 1]].view(B, 4 * A, H, W) for l, (_, H, W) in enumerate(maps)])


class BoxHead:
    """box_head(roi_feats (R,C,P,P)) -> (class_logits (R,K), box_regression (R,4K)): flatten in (c, y, x) order, relu(fc6), relu(fc7), predictors"""

    def __init__(self, fc6, fc7, pred):
        self.fc6, self.fc7, self.pred = fc6, fc7, pred
        self.K = pred.n_split
        if pred.c_out != 5 * self.K:
            raise ValueError(f'box_predictor.bbox_pred must have 4 x the {self.K} outputs of cls_score, got {pred.c_out - self.K}')
        if fc7.c_in != fc6.c_out or pred.c_in != fc7.c_out:
            raise ValueError(f'box head widths do not chain: fc6 -> {fc6.c_out}, fc7 {fc7.c_in} -> {fc7.c_out}, predictors {pred.c_in}')

    def __call__(self, roi_feats):
        if not torch.is_tensor(roi_feats) or roi_feats.dim() != 4:
            raise ValueError(f'roi_feats must be (R,C,P,P), got {tuple(roi_feats.shape) if torch.is_tensor(roi_feats) else type(roi_feats).__name__}')
        flat = roi_feats.contiguous().view(roi_feats.shape[0], int(roi_feats.shape[1] * roi_feats.shape[2] * roi_feats.shape[3]))      # torch's (c, y, x) order
        flat = _on_device(_check_input(flat, 'roi_feats, flattened,', 2, self.fc6.c_in, '(R, C x P x P)'), 'roi_feats')
        R, dev, K = int(flat.shape[0]), flat.device, self.K
        for layer in (self.fc6, self.fc7, self.pred):
            _ready(layer, dev)
        rows = flat
        if self.fc6.dtype != torch.float32:
            rows = _rows(R, self.fc6.c_in, self.fc6, dev)
            _pack(flat, rows, R, self.fc6.c_in, 1, self.fc6.dtype)
        maps = [(R, 1, 1)]
        h6 = _gemm(self.fc6, rows, maps, _lib.HEAD_STORE_ROWS, _rows(R, self.fc6.c_out, self.fc6, dev))
        h7 = _gemm(self.fc7, h6, maps, _lib.HEAD_STORE_ROWS, _rows(R, self.fc7.c_out, self.fc7, dev))
        logits = torch.empty((R, K), dtype=torch.float32, device=dev)
        boxes = torch.empty((R, 4 * K), dtype=torch.float32, device=dev)
        _gemm(self.pred, h7, maps, _lib.HEAD_STORE_NCHW, logits, boxes, n_split=K)
        return logits, boxes


class MaskHead:
    """mask_head(roi_feats (D,C,H,W)) -> (D,K,2H,2W) logits: four 3x3 conv + ReLU, the deconv + ReLU, the 1x1"""

    def __init__(self, convs, deconv, logits):
        self.convs, self.deconv, self.logits = list(convs), deconv, logits
        chain = self.convs + [deconv]
        for a, b in zip(chain[:-1], chain[1:]):
            if b.c_in != a.n_out:
                raise ValueError(f'mask head widths do not chain: {a.n_out} channels into a layer of {b.c_in}')
        if logits.c_in != deconv.n_out:
            raise ValueError(f'mask head widths do not chain: {deconv.n_out} channels into mask_fcn_logits of {logits.c_in}')

    def __call__(self, roi_feats):
        x = _on_device(_check_input(roi_feats, 'roi_feats', 4, self.convs[0].c_in, '(D,C,H,W)'), 'roi_feats')
        D, C, H, W = (int(v) for v in x.shape)
        dev = x.device
        if D and H * W < 1:
            raise ValueError(f'roi_feats must have at least one cell, got {tuple(x.shape)}')
        for layer in self.convs + [self.deconv, self.logits]:
            _ready(layer, dev)
        maps = [(D, H, W)]
        rows = _rows(D * H * W, C, self.convs[0], dev)
        _pack(x, rows, D, C, H * W, self.convs[0].dtype)
        for layer in self.convs:
            rows = _gemm(layer, rows, maps, _lib.HEAD_STORE_ROWS, _rows(D * H * W, layer.c_out, layer, dev))
        up = _gemm(self.deconv, rows, maps, _lib.HEAD_STORE_DECONV_ROWS, _rows(4 * D * H * W, self.deconv.n_out, self.deconv, dev))
        out = torch.empty((D, self.logits.c_out, 2 * H, 2 * W), dtype=torch.float32, device=dev)
        return _gemm(self.logits, up, [(D, 2 * H, 2 * W)], _lib.HEAD_STORE_NCHW, out)


class DetectorHeads:
    """The three heads as callables with the signatures detector_rpn.detections_from_features documents: .rpn_head, .box_head, .mask_head
    (None without a mask branch).  Weights are packed once, here."""

    def __init__(self, params, dtype=torch.float32, device=None):
        """params: {key: (weight, bias)} under the names of a torchvision 0.4.2 Mask R-CNN state_dict, without the '.weight' / '.bias'"""
        dtype = _dtype(dtype)
        kw = dict(dtype=dtype, device=device)
        p = params
        self.dtype = dtype
        self.rpn_head = RpnHead(HeadLayer.conv(*p[RPN_KEYS[0]], relu=True, **kw), HeadLayer.siblings(p[RPN_KEYS[1]], p[RPN_KEYS[2]], 'conv', **kw))
        self.box_head = BoxHead(HeadLayer.linear(*p[BOX_KEYS[0]], relu=True, **kw), HeadLayer.linear(*p[BOX_KEYS[1]], relu=True, **kw),
                                HeadLayer.siblings(p[BOX_KEYS[2]], p[BOX_KEYS[3]], 'linear', **kw))
        self.mask_head = None
        if MASK_KEYS[0] in p:
            self.mask_head = MaskHead([HeadLayer.conv(*p[k], relu=True, **kw) for k in MASK_KEYS[:4]], HeadLayer.deconv(*p[MASK_KEYS[4]], relu=True, **kw),
                                      HeadLayer.conv(*p[MASK_KEYS[5]], relu=False, **kw))

    def layers(self):
        """every packed layer, in a fixed order (tests compare their bytes)"""
        out = [self.rpn_head.conv, self.rpn_head.pred, self.box_head.fc6, self.box_head.fc7, self.box_head.pred]
        if self.mask_head is not None:
            out += self.mask_head.convs + [self.mask_head.deconv, self.mask_head.logits]
        return out

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float32, device=None):
        """a Mask R-CNN state_dict as it is: the trunk's and the FPN's keys are ignored, a missing head key is a KeyError naming it"""
        params = {}
        for k in RPN_KEYS + BOX_KEYS + MASK_KEYS:
            for part in ('weight', 'bias'):
                if f'{k}.{part}' not in sd:
                    raise KeyError(f'{k}.{part}')
            params[k] = (sd[f'{k}.weight'], sd[f'{k}.bias'])
        return cls(params, dtype, device)

    @classmethod
    def from_modules(cls, rpn_head, box_head, box_predictor, mask_head=None, mask_predictor=None, dtype=torch.float32, device=None):
        """the same from modules, duck-typed on torchvision's attribute names (conv, cls_logits, bbox_pred; fc6, fc7; cls_score, bbox_pred;
        mask_fcn1..4; conv5_mask, mask_fcn_logits)"""
        if (mask_head is None) != (mask_predictor is None):
            raise ValueError('mask_head and mask_predictor go together: give both or neither')
        named = [(RPN_KEYS[0], rpn_head, 'conv'), (RPN_KEYS[1], rpn_head, 'cls_logits'), (RPN_KEYS[2], rpn_head, 'bbox_pred'),
                 (BOX_KEYS[0], box_head, 'fc6'), (BOX_KEYS[1], box_head, 'fc7'), (BOX_KEYS[2], box_predictor, 'cls_score'),
                 (BOX_KEYS[3], box_predictor, 'bbox_pred')]
        if mask_head is not None:
            named += [(MASK_KEYS[i], mask_head, f'mask_fcn{i + 1}') for i in range(4)]
            named += [(MASK_KEYS[4], mask_predictor, 'conv5_mask'), (MASK_KEYS[5], mask_predictor, 'mask_fcn_logits')]
        params = {}
        for key, module, attr in named:
            m = getattr(module, attr)
            params[key] = (m.weight, m.bias)
        if device is None:
            device = rpn_head.conv.weight.device
            device = device if device.type != 'cpu' else None
        return cls(params, dtype, device)

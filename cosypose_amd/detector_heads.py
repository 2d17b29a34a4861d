"""The detector's heads on the matrix pipe: Mask R-CNN's RPN head, box head + predictor and mask head + predictor (torchvision 0.4.2), the
convolutions and linears between the FPN and detector.detections_from_heads.  By default inference only (HIP: csrc/kernels_dethead.hip, cosy_head_pack and
cosy_head_conv).  DetectorHeads(..., trainable=True) are float32 heads with parameters and a backward on the same matrix pipe, behind autograd
(HIP: csrc/kernels_detbwd.hip, which the trunk's backward, detector_trunk_backward.py (section 29), runs too); with
train_dtype=torch.bfloat16 their rows and packed weights are bfloat16 under the float32 parameters (section 32; csrc/kernels_detbwd16.hip).

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


def k_block(dtype):
    """channels of one block of a GEMM's reduction (csrc/dethead_device.h: KB): one MFMA step of the rows' type"""
    return 16 if dtype == torch.float32 else 32


def pack_weight(w, dtype):
    """(N, taps, C_in) float32 CPU -> the fragment order cosy_head_conv reads (cosyhip.h): [N_pad / 16][tap][k-block][lane][element], zero padded"""
    N, taps, C = (int(v) for v in w.shape)
    KB = k_block(dtype)
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


def _pad8(n):
    return -(-n // 8) * 8


def transposed_weight(kind, weight):
    """a parameter in torchvision's layout (CPU) -> (C_in, taps, O) float32, the weight of the data gradient's GEMM: rows c, reduction o;
    conv: the taps in reverse order (the gradient at cell - tap meets tap); deconv (C_in, O, 2, 2): the four taps (dy, dx) ascending.
    pack_weight(transposed_weight(...), torch.float32) is the host statement of what cosy_head_weight_pack writes as `bwd`."""
    w = weight.detach().to(device='cpu', dtype=torch.float32)
    if kind == 'linear':
        return w.t().reshape(w.shape[1], 1, w.shape[0])
    if kind == 'conv':
        return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], w.shape[2] * w.shape[3], w.shape[0])
    if kind == 'deconv':
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], 4, w.shape[1])
    raise ValueError(f'kind must be conv, linear or deconv, got {kind}')


class PackedOnDevice:
    """What a trainable layer of the heads and one of the trunk share: parameters() on self.device, and the packings w / bias / w_t that one
    launch writes from them on the device.  A subclass states its layer once, as pack_args(), and how its entry point takes it, as _pack()."""

    def pack_args(self):
        """-> (w0, b0, w1, b1, scale, ksize, c_in, n0, n1): the layer as a weight pack takes it (cosyhip.h: cosy_head_weight_pack; a trunk
        layer is the case n1 = 0, b0 = shift); tensors or None, ksize 2 for ConvTranspose2d(2, 2)"""
        raise NotImplementedError

    @staticmethod
    def packed_sizes(ksize, c_in, n0, n1, dtype):
        """-> the elements of (w, bias, w_t) that a pack writes: csrc/detbwd_device.h's pack_sizes"""
        KB, O = k_block(dtype), n0 + n1
        rows_f, taps_f, taps_b = (4 * O if ksize == 2 else O), (9 if ksize == 3 else 1), {1: 1, 2: 4, 3: 9}[ksize]
        NPf, NPb = -(-rows_f // 64) * 64, -(-c_in // 64) * 64
        return NPf * taps_f * (-(-c_in // KB) * KB), NPf, NPb * taps_b * (-(-O // KB) * KB)

    def _alloc_packings(self):
        n_w, n_bias, n_wt = self.packed_sizes(*self.pack_args()[5:], self.dtype)
        self.w = torch.empty(n_w, dtype=self.dtype, device=self.device)
        self.bias = torch.empty(n_bias, dtype=torch.float32, device=self.device)
        self.w_t = torch.empty(n_wt, dtype=self.dtype, device=self.device)
        self.versions = None

    def refresh(self, dev=None):
        """pack on the device when a parameter's _version (or its storage) has moved since the last pack, and not otherwise"""
        if dev is not None and torch.device(dev) != self.device:
            raise ValueError(f'the input lives on {dev}, the parameters on {self.device}: build the {self.owner} with device={dev!s}')
        now = tuple((p._version, p.data_ptr()) for p in self.parameters())
        if now != self.versions:
            with torch.cuda.device(self.device):
                self._pack()
            self.versions = now
            self.counter[0] += 1
        return self


class TrainableLayer(PackedOnDevice):
    """A layer of trainable heads: its parameters are float32 torch.nn.Parameters on the device in torchvision's layout
    (one (weight, bias) pair, or the two siblings of one GEMM); w / bias (what cosy_head_conv reads) and w_t (the transposed, tap-flipped
    packing the data gradient reads) are written by cosy_head_weight_pack on the device, when a parameter has moved since the last pack.
    kind, ksize, relu, c_in, c_out, n_out as HeadLayer; grad_ksize: 3, 1, or 2 for the deconvolution; n_grad: the outputs o of the gradient
    rows (deconv: C_o, else c_out).  dtype: the type of the rows and of w / w_t (the parameters are float32 whatever it is); torch.bfloat16
    (section 32) packs through cosy_head_weight_pack16: w holds the bytes of the host packing of the weight rounded to bfloat16."""
    dtype, owner = torch.float32, 'heads'

    def __init__(self, kind, pairs, relu, device, counter=None, dtype=torch.float32):
        if device is None or torch.device(device).type != 'cuda':
            raise ValueError(f'trainable heads live on the ROCm device: give device=, got {device}')
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'the rows of trainable heads are float32 or bfloat16, got {dtype}')
        self.dtype = dtype
        self.kind, self.relu, self.device = kind, bool(relu), torch.device(device)
        self.counter = counter if counter is not None else [0]
        self.pairs = []
        for w, b in pairs:
            if b is None:
                b = torch.zeros(w.shape[1] if kind == 'deconv' else w.shape[0])
            self.pairs.append(tuple(p if isinstance(p, torch.nn.Parameter) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
                                    else torch.nn.Parameter(p.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()) for p in (w, b)))
        w0 = self.pairs[0][0]
        self.device = w0.device                                   # 'cuda' resolved to the device the parameters landed on
        dims = {'conv': 4, 'linear': 2, 'deconv': 4}[kind]
        for w, b in self.pairs:
            if w.dim() != dims or b.dim() != 1:
                raise ValueError(f'a {kind} layer takes a {dims}-d weight and a 1-d bias, got {tuple(w.shape)} and {tuple(b.shape)}')
        if kind == 'deconv':
            if tuple(w0.shape[2:]) != (2, 2) or len(self.pairs) != 1:
                raise ValueError(f'a deconv layer is one ConvTranspose2d(k=2, s=2), got a kernel of {tuple(w0.shape[2:])}')
            self.c_in, self.n_grad, self.ksize, self.grad_ksize = int(w0.shape[0]), int(w0.shape[1]), 1, 2
            self.c_out, self.n_out = 4 * self.n_grad, self.n_grad
            if self.n_grad % 8:
                raise ValueError(f'a trainable deconv layer has a multiple of 8 output channels, got {self.n_grad}')
        else:
            k = int(w0.shape[2]) if kind == 'conv' else 1
            if k not in (1, 3) or (kind == 'conv' and w0.shape[3] != k):
                raise ValueError(f'a conv layer is 3x3 or 1x1, got a kernel of {tuple(w0.shape[2:])}')
            if any(tuple(w.shape[1:]) != tuple(w0.shape[1:]) for w, _ in self.pairs):
                raise ValueError(f'sibling layers read the same input, got weights {[tuple(w.shape) for w, _ in self.pairs]}')
            self.c_in, self.ksize, self.grad_ksize = int(w0.shape[1]), k, k
            self.c_out = self.n_out = self.n_grad = sum(int(w.shape[0]) for w, _ in self.pairs)
        for w, b in self.pairs:
            if int(b.shape[0]) != int(w.shape[1] if kind == 'deconv' else w.shape[0]):
                raise ValueError(f'bias must be ({int(w.shape[1] if kind == "deconv" else w.shape[0])}), got {tuple(b.shape)}')
        if self.c_in < 8 or self.c_in % 8:
            raise ValueError(f'{kind} layer: the reduction length {self.c_in} must be a positive multiple of 8 (it is not padded silently)')
        if len(self.pairs) == 2:
            self.n_split = int(w0.shape[0])
        self._alloc_packings()

    def parameters(self):
        return [p for pair in self.pairs for p in pair]

    def pack_args(self):
        (w0, b0), (w1, b1) = self.pairs[0], (self.pairs[1] if len(self.pairs) == 2 else (None, None))
        n0 = int(w0.shape[1] if self.kind == 'deconv' else w0.shape[0])
        return w0, b0, w1, b1, None, self.grad_ksize, self.c_in, n0, self.n_grad - n0

    def _pack(self):
        w0, b0, w1, b1, _, ksize, c_in, n0, n1 = self.pack_args()
        _lib.check(_lib.rows_entry('cosy_head_weight_pack', self.dtype)(_lib.ptr(w0), _lib.ptr(b0), _lib.ptr(w1), _lib.ptr(b1), ksize, c_in, n0, n1, _lib.ptr(self.w),
                                                                      _lib.ptr(self.bias), _lib.ptr(self.w_t), _lib.stream()))

    @classmethod
    def conv(cls, weight, bias=None, relu=False, device=None, counter=None, dtype=torch.float32):
        return cls('conv', [(weight, bias)], relu, device, counter, dtype)

    @classmethod
    def linear(cls, weight, bias=None, relu=False, device=None, counter=None, dtype=torch.float32):
        return cls('linear', [(weight, bias)], relu, device, counter, dtype)

    @classmethod
    def deconv(cls, weight, bias=None, relu=False, device=None, counter=None, dtype=torch.float32):
        return cls('deconv', [(weight, bias)], relu, device, counter, dtype)

    @classmethod
    def siblings(cls, first, second, kind, device=None, counter=None, dtype=torch.float32):
        return cls(kind, [tuple(first), tuple(second)], False, device, counter, dtype)


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


def _on_device(x, name, trainable=False):
    """after every shape and dtype check, before anything touches the library"""
    if not x.is_cuda:
        raise ValueError(f'{name} must live on the ROCm device (got a CPU tensor); there is no CPU fallback')
    if torch.is_grad_enabled() and x.requires_grad and not trainable:
        raise RuntimeError(f'{name} requires grad: DetectorHeads is inference only, training keeps the torch.nn modules and autograd '
                           '(detector_train.detector_losses); call it under torch.no_grad() or detach the input')
    return x.contiguous()


def _ready(layer, dev):
    """the layer's weights on the input's device: a layer packed without a device is uploaded on its first use and stays there; a layer
    that lives on another device is refused (a silent re-upload would move the weights under another stream's feet)"""
    if isinstance(layer, TrainableLayer):
        return layer.refresh(dev)
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


def _describe(d, maps):
    """the maps of a launch in its descriptor; maps: [(images, H, W)] per level, in row order -> the rows they hold"""
    d.n_levels = len(maps)
    row = 0
    for l, (n, H, W) in enumerate(maps):
        d.row_start[l], d.H[l], d.W[l] = row, H, W
        row += n * H * W
        if row > MAX_ROWS:
            raise ValueError(f'{row} rows (cells of all maps) exceed the limit of 2^30 per launch')
    d.row_start[len(maps)] = row
    return row


def _gemm(layer, x_rows, maps, store, out, out1=None, n_split=None):
    """one launch of layer over x_rows; maps: [(images, H, W)] per level, in row order"""
    d = _lib.HeadLayer()
    d.x, d.w, d.bias, d.out, d.out1 = _lib.ptr(x_rows), _lib.ptr(layer.w), _lib.ptr(layer.bias), _lib.ptr(out), _lib.ptr(out1)
    d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store = _DTYPES[layer.dtype], layer.ksize, layer.c_in, layer.c_out, int(layer.relu), store
    d.n_split = layer.c_out if n_split is None else n_split
    if _describe(d, maps):
        _lib.check(_lib.lib().cosy_head_conv(ctypes.byref(d), _lib.stream()))
    return out


def conv_layer(x, layer):
    """One layer through the kernel.  conv: x (B,C,H,W) -> (B,N,H,W); linear: x (M,K) -> (M,N); deconv: x (B,C,H,W) -> (B,N/4,2H,2W).
    x float32, contiguous, on the device; the result is float32 NCHW.  x is rounded to the layer's storage type on the way in."""
    if not isinstance(layer, (HeadLayer, TrainableLayer)):
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


# ---- backward (DESIGN.md sections 28 and 32): rows of the layer's dtype, the gradient g of a layer is taken at its PRE-activation output -----
def wgrad_slab_rows(M):
    """cells of one slab of the weight gradient of M cells (the library's; tests sit on its edges)"""
    return int(_lib.lib().cosy_head_wgrad_slab_rows(int(M)))


def _grad_pack(g0, g1, rows, B, n0, n1, HW):
    """NCHW float32 gradients of a sibling pair (or of one tensor, n1 = 0; None: zeros) -> rows (B HW, pad8(n0 + n1)) of rows' own type
    (float32, or bfloat16: rounded to nearest even), one launch"""
    for g, n in ((g0, n0), (g1, n1)):
        if g is not None and (g.dtype != torch.float32 or g.numel() != B * n * HW or not g.is_cuda):
            raise ValueError(f'a gradient of {B} x {n} x {HW} float32 values on the device was expected, got {tuple(g.shape)} {g.dtype} on {g.device}')
    if B:
        pack = _lib.rows_entry('cosy_head_grad_pack', rows.dtype)
        _lib.check(pack(_lib.ptr(None if g0 is None else g0.contiguous()), _lib.ptr(None if g1 is None else g1.contiguous()), _lib.ptr(rows), B, n0, n1, HW,
                        _lib.stream()))
    return rows


def _dgrad(layer, g_rows, maps, store, out, y=None):
    """the data gradient of layer from its gradient rows; maps: those of g_rows.  y: the stored rows of the layer below (the ReLU mask).
    A row store writes rows of the layer's dtype, an NCHW store float32 whatever it is"""
    d = _lib.HeadLayer()
    d.x, d.w, d.out = _lib.ptr(g_rows), _lib.ptr(layer.w_t), _lib.ptr(out)
    d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store = _DTYPES[layer.dtype], layer.grad_ksize, int(g_rows.shape[1]), layer.c_in, 0, store
    d.n_split = layer.c_in
    if _describe(d, maps):
        _lib.check(_lib.rows_entry('cosy_head_dgrad', layer.dtype)(ctypes.byref(d), _lib.ptr(y), _lib.stream()))
    return out


def _wgrad_buffers(layer, M, ksize, c_out):
    """what a weight gradient over M cells writes: the gradients in the parameters' layout, the slabs' workspace and its bytes"""
    need = int(_lib.lib().cosy_head_wgrad_workspace_bytes(M, ksize, layer.c_in, c_out))
    if M and not need:
        raise ValueError(f'the weight gradient of {M} cells, c_in={layer.c_in}, c_out={c_out} does not fit the library\'s limits')
    return [torch.empty_like(p) for p in layer.parameters()], torch.empty(max(need // 4, 4), dtype=torch.float32, device=layer.device), need


def _wgrad(layer, x_rows, g_rows, maps):
    """-> [dW, db] per parameter pair of layer, float32 in the parameters' own layout; maps: those of x_rows"""
    d = _lib.HeadLayer()
    d.x = _lib.ptr(x_rows)
    d.dtype, d.ksize, d.c_in, d.c_out = _DTYPES[layer.dtype], layer.grad_ksize, layer.c_in, layer.n_grad
    d.n_split = getattr(layer, 'n_split', layer.n_grad)
    out, ws, need = _wgrad_buffers(layer, _describe(d, maps), layer.grad_ksize, layer.n_grad)
    wgrad = _lib.rows_entry('cosy_head_wgrad', layer.dtype)
    _lib.check(wgrad(ctypes.byref(d), _lib.ptr(g_rows), *[_lib.ptr(t) for t in (out + [None, None])[:4]], _lib.ptr(ws), need, _lib.stream()))
    return out


def layer_backward(layer, x, grad, need_dx=True):
    """One TrainableLayer's backward through the kernels.  x as conv_layer takes it; grad: the gradient at the layer's PRE-activation output,
    float32 with the shape of conv_layer's result (the layer's own ReLU is not applied: in a head the launch above masks).
    -> dX (float32, the shape of x; None without need_dx), [dW, db (, dW, db of the second sibling)] in the parameters' layout"""
    if not isinstance(layer, TrainableLayer):
        raise ValueError(f'layer must be a TrainableLayer, got {type(layer).__name__}')
    linear = layer.kind == 'linear'
    x = _on_device(_check_input(x, 'x', 2 if linear else 4, layer.c_in, '(M,K)' if linear else '(B,C,H,W)'), 'x', True).detach()
    dev = x.device
    _ready(layer, dev)
    B, C, H, W = (int(v) for v in x.shape) if not linear else (int(x.shape[0]), layer.c_in, 1, 1)
    up = 2 if layer.kind == 'deconv' else 1
    want = (B, layer.n_out) if linear else (B, layer.n_out, up * H, up * W)
    if not torch.is_tensor(grad) or tuple(grad.shape) != want or grad.dtype != torch.float32 or not grad.is_cuda:
        raise ValueError(f'grad must be a float32 tensor of shape {want} on the device')
    rows = x
    if not linear or layer.dtype != torch.float32:
        rows = _rows(B * H * W, C, layer, dev)
        _pack(x, rows, B, C, H * W, layer.dtype)
    g = _grad_pack(grad.detach(), None, _rows(B * up * H * up * W, _pad8(layer.n_out), layer, dev), B, layer.n_out, 0, up * H * up * W)
    grads = _wgrad(layer, rows, g, [(B, H, W)])
    dx = None
    if need_dx:
        dx = _dgrad(layer, g, [(B, up * H, up * W)], _lib.HEAD_STORE_NCHW, torch.empty_like(x))
    return dx, grads


def _wants_grad(head, inputs):
    return head.trainable and torch.is_grad_enabled() and any(t.requires_grad for t in list(inputs) + head.parameters())


def _once(name):
    if torch.is_grad_enabled():
        raise RuntimeError(f'DetectorHeads.{name}: double backward is not built (the backward of the heads\' backward has no kernel); '
                           'call backward() without create_graph')


def _g(t):
    return None if t is None else t.contiguous()


def _note(head, keep, **rows):
    """head.keep_rows (the tests): the rows the forward kept and every gradient row buffer of this backward, under the names of its launches"""
    if getattr(head, 'keep_rows', False):
        head.last_rows = dict(keep, **rows)


class _RpnFn(torch.autograd.Function):
    """rpn_head as one node: forward = RpnHead._forward's launches; backward = per level one gradient pack, then for the sibling 1x1 GEMM and
    the 3x3 conv the weight gradient and the data gradient (the first masked by the stored hidden rows, the second stored NCHW per level)"""

    @staticmethod
    def forward(ctx, head, L, *tensors):
        keep = {}
        obj, dlt = head._forward(list(tensors[:L]), keep)
        ctx.head, ctx.keep, ctx.L = head, keep, L
        return tuple(obj) + tuple(dlt)

    @staticmethod
    def backward(ctx, *grads):
        _once('rpn_head')
        head, k, L = ctx.head, ctx.keep, ctx.L
        maps, starts, A = k['maps'], k['starts'], head.A
        M, dev = starts[-1], k['x'].device
        g = _rows(M, _pad8(5 * A), head.conv, dev)
        for l, (B, H, W) in enumerate(maps):
            _grad_pack(_g(grads[l]), _g(grads[L + l]), g[starts[l]:starts[l + 1]], B, A, 4 * A, H * W)
        d_pred = _wgrad(head.pred, k['hidden'], g, maps)
        gh = _dgrad(head.pred, g, maps, _lib.HEAD_STORE_ROWS, _rows(M, head.conv.c_out, head.conv, dev), y=k['hidden'])
        d_conv = _wgrad(head.conv, k['x'], gh, maps)
        dfeat = [None] * L
        if any(ctx.needs_input_grad[2:2 + L]):
            C = head.conv.c_in
            flat = _dgrad(head.conv, gh, maps, _lib.HEAD_STORE_NCHW, torch.empty(C * M, dtype=torch.float32, device=dev))
            dfeat = [flat[C * starts[l]:C * starts[l + 1]].view(B, C, H, W) if ctx.needs_input_grad[2 + l] else None for l, (B, H, W) in enumerate(maps)]
        _note(head, k, g=g, gh=gh)
        return (None, None) + tuple(dfeat) + tuple(d_conv) + tuple(d_pred)


class _BoxFn(torch.autograd.Function):
    """box_head as one node: the predictors, fc7 and fc6 backwards, each a weight gradient and a data gradient masked by the rows below"""

    @staticmethod
    def forward(ctx, head, flat, *params):
        keep = {}
        out = head._forward(flat, keep)
        ctx.head, ctx.keep = head, keep
        return out

    @staticmethod
    def backward(ctx, g_logits, g_boxes):
        _once('box_head')
        head, k = ctx.head, ctx.keep
        maps, K, x = k['maps'], head.K, k['x']
        R, dev = int(x.shape[0]), x.device
        new = lambda n: _rows(R, n, head.fc6, dev)
        g = _grad_pack(_g(g_logits), _g(g_boxes), new(_pad8(5 * K)), R, K, 4 * K, 1)
        d_pred = _wgrad(head.pred, k['h7'], g, maps)
        g7 = _dgrad(head.pred, g, maps, _lib.HEAD_STORE_ROWS, new(head.fc7.c_out), y=k['h7'])
        d_fc7 = _wgrad(head.fc7, k['h6'], g7, maps)
        g6 = _dgrad(head.fc7, g7, maps, _lib.HEAD_STORE_ROWS, new(head.fc6.c_out), y=k['h6'])
        d_fc6 = _wgrad(head.fc6, x, g6, maps)
        dx = None
        if ctx.needs_input_grad[1]:
            dx = _dgrad(head.fc6, g6, maps, _lib.HEAD_STORE_NCHW, torch.empty((R, head.fc6.c_in), dtype=torch.float32, device=dev))
        _note(head, k, g=g, g7=g7, g6=g6)
        return (None, dx) + tuple(d_fc6) + tuple(d_fc7) + tuple(d_pred)


class _MaskFn(torch.autograd.Function):
    """mask_head as one node: the 1x1 logits, the deconvolution (four stride-2 taps) and the four 3x3 convs, last to first"""

    @staticmethod
    def forward(ctx, head, x, *params):
        keep = {}
        out = head._forward(x, keep)
        ctx.head, ctx.keep, ctx.shape = head, keep, tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        _once('mask_head')
        head, k = ctx.head, ctx.keep
        (D, H, W), = k['maps']
        maps, maps2, rows, up, dev = k['maps'], [(D, 2 * H, 2 * W)], k['rows'], k['up'], k['up'].device
        M, K = D * H * W, head.logits.c_out
        new = lambda m, n: _rows(m, n, head.deconv, dev)
        g = _grad_pack(_g(g_out), None, new(4 * M, _pad8(K)), D, K, 0, 4 * H * W)
        d_logits = _wgrad(head.logits, up, g, maps2)
        g_up = _dgrad(head.logits, g, maps2, _lib.HEAD_STORE_ROWS, new(4 * M, head.deconv.n_out), y=up)
        d_deconv = _wgrad(head.deconv, rows[-1], g_up, maps)
        g_cur = _dgrad(head.deconv, g_up, maps2, _lib.HEAD_STORE_ROWS, new(M, head.deconv.c_in), y=rows[-1])
        d_convs, dx, g_convs = [], None, [g_cur]
        for i in range(len(head.convs) - 1, -1, -1):
            layer = head.convs[i]
            d_convs = _wgrad(layer, rows[i], g_cur, maps) + d_convs
            if i:
                g_cur = _dgrad(layer, g_cur, maps, _lib.HEAD_STORE_ROWS, new(M, layer.c_in), y=rows[i])
                g_convs.insert(0, g_cur)
            elif ctx.needs_input_grad[1]:
                dx = _dgrad(layer, g_cur, maps, _lib.HEAD_STORE_NCHW, torch.empty(ctx.shape, dtype=torch.float32, device=dev))
        _note(head, k, g=g, g_up=g_up, g_convs=g_convs)
        return (None, dx) + tuple(d_convs) + tuple(d_deconv) + tuple(d_logits)


# ---- the three heads -----------------------------------------------------------------------------------------------------------------
class RpnHead:
    """rpn_head(features) -> (objectness, bbox_deltas): per level (B,A,H,W) and (B,4A,H,W) float32, views of two flat buffers"""

    def __init__(self, conv, pred):
        self.conv, self.pred = conv, pred
        self.trainable = isinstance(conv, TrainableLayer)
        self.A = pred.n_split
        if pred.c_out != 5 * self.A:
            raise ValueError(f'rpn.head.bbox_pred must have 4 x the {self.A} outputs of cls_logits, got {pred.c_out - self.A}')

    def parameters(self):
        return self.conv.parameters() + self.pred.parameters() if self.trainable else []

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
        feats = [_on_device(f, f'features[{l}]', self.trainable) for l, f in enumerate(feats)]
        if _wants_grad(self, feats):
            out = _RpnFn.apply(self, len(feats), *feats, *self.parameters())
            return list(out[:len(feats)]), list(out[len(feats):])
        return self._forward(feats)

    def _forward(self, feats, keep=None):
        B = int(feats[0].shape[0])
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
        if keep is not None:
            keep.update(x=x, hidden=hidden, maps=maps, starts=starts)
        return ([obj[A * starts[l]:A * starts[l + 1]].view(B, A, H, W) for l, (_, H, W) in enumerate(maps)],
                [dlt[4 * A * starts[l]:4 * A * starts[l + 1]].view(B, 4 * A, H, W) for l, (_, H, W) in enumerate(maps)])


class BoxHead:
    """box_head(roi_feats (R,C,P,P)) -> (class_logits (R,K), box_regression (R,4K)): flatten in (c, y, x) order, relu(fc6), relu(fc7), predictors"""

    def __init__(self, fc6, fc7, pred):
        self.fc6, self.fc7, self.pred = fc6, fc7, pred
        self.trainable = isinstance(fc6, TrainableLayer)
        self.K = pred.n_split
        if pred.c_out != 5 * self.K:
            raise ValueError(f'box_predictor.bbox_pred must have 4 x the {self.K} outputs of cls_score, got {pred.c_out - self.K}')
        if fc7.c_in != fc6.c_out or pred.c_in != fc7.c_out:
            raise ValueError(f'box head widths do not chain: fc6 -> {fc6.c_out}, fc7 {fc7.c_in} -> {fc7.c_out}, predictors {pred.c_in}')

    def parameters(self):
        return self.fc6.parameters() + self.fc7.parameters() + self.pred.parameters() if self.trainable else []

    def __call__(self, roi_feats):
        if not torch.is_tensor(roi_feats) or roi_feats.dim() != 4:
            raise ValueError(f'roi_feats must be (R,C,P,P), got {tuple(roi_feats.shape) if torch.is_tensor(roi_feats) else type(roi_feats).__name__}')
        flat = roi_feats.contiguous().view(roi_feats.shape[0], int(roi_feats.shape[1] * roi_feats.shape[2] * roi_feats.shape[3]))      # torch's (c, y, x) order
        flat = _on_device(_check_input(flat, 'roi_feats, flattened,', 2, self.fc6.c_in, '(R, C x P x P)'), 'roi_feats', self.trainable)
        if _wants_grad(self, [flat]):
            return _BoxFn.apply(self, flat, *self.parameters())
        return self._forward(flat)

    def _forward(self, flat, keep=None):
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
        if keep is not None:
            keep.update(x=rows, h6=h6, h7=h7, maps=maps)
        return logits, boxes


class MaskHead:
    """mask_head(roi_feats (D,C,H,W)) -> (D,K,2H,2W) logits: four 3x3 conv + ReLU, the deconv + ReLU, the 1x1"""

    def __init__(self, convs, deconv, logits):
        self.convs, self.deconv, self.logits = list(convs), deconv, logits
        self.trainable = isinstance(deconv, TrainableLayer)
        chain = self.convs + [deconv]
        for a, b in zip(chain[:-1], chain[1:]):
            if b.c_in != a.n_out:
                raise ValueError(f'mask head widths do not chain: {a.n_out} channels into a layer of {b.c_in}')
        if logits.c_in != deconv.n_out:
            raise ValueError(f'mask head widths do not chain: {deconv.n_out} channels into mask_fcn_logits of {logits.c_in}')

    def parameters(self):
        return [p for layer in self.convs + [self.deconv, self.logits] for p in layer.parameters()] if self.trainable else []

    def __call__(self, roi_feats):
        x = _on_device(_check_input(roi_feats, 'roi_feats', 4, self.convs[0].c_in, '(D,C,H,W)'), 'roi_feats', self.trainable)
        if x.shape[0] and x.shape[2] * x.shape[3] < 1:
            raise ValueError(f'roi_feats must have at least one cell, got {tuple(x.shape)}')
        if _wants_grad(self, [x]):
            return _MaskFn.apply(self, x, *self.parameters())
        return self._forward(x)

    def _forward(self, x, keep=None):
        D, C, H, W = (int(v) for v in x.shape)
        dev = x.device
        for layer in self.convs + [self.deconv, self.logits]:
            _ready(layer, dev)
        maps = [(D, H, W)]
        rows = _rows(D * H * W, C, self.convs[0], dev)
        _pack(x, rows, D, C, H * W, self.convs[0].dtype)
        stored = [rows]
        for layer in self.convs:
            rows = _gemm(layer, rows, maps, _lib.HEAD_STORE_ROWS, _rows(D * H * W, layer.c_out, layer, dev))
            stored.append(rows)
        up = _gemm(self.deconv, rows, maps, _lib.HEAD_STORE_DECONV_ROWS, _rows(4 * D * H * W, self.deconv.n_out, self.deconv, dev))
        out = torch.empty((D, self.logits.c_out, 2 * H, 2 * W), dtype=torch.float32, device=dev)
        if keep is not None:
            keep.update(rows=stored, up=up, maps=maps)
        return _gemm(self.logits, up, [(D, 2 * H, 2 * W)], _lib.HEAD_STORE_NCHW, out)


class DetectorHeads:
    """The three heads as callables with the signatures detector_rpn.detections_from_features documents: .rpn_head, .box_head, .mask_head
    (None without a mask branch).  Weights are packed once, here."""

    def __init__(self, params, dtype=torch.float32, device=None, trainable=False, train_dtype=None):
        """params: {key: (weight, bias)} under the names of a torchvision 0.4.2 Mask R-CNN state_dict, without the '.weight' / '.bias'.
        trainable: the parameters become float32 torch.nn.Parameters on the device and the three heads autograd nodes (see _init_trainable);
        train_dtype: the type of their rows and packed weights, None / torch.float32 (section 28) or torch.bfloat16 (section 32)"""
        from .detector_trunk_backward import check_train_dtype
        dtype = _dtype(dtype)
        kw = dict(dtype=dtype, device=device)
        p = params
        self.dtype = dtype
        self.trainable = bool(trainable)
        self.train_dtype = check_train_dtype(self.trainable, train_dtype, 'heads')
        if self.trainable:
            return self._init_trainable(p, dtype, device)
        self.rpn_head = RpnHead(HeadLayer.conv(*p[RPN_KEYS[0]], relu=True, **kw), HeadLayer.siblings(p[RPN_KEYS[1]], p[RPN_KEYS[2]], 'conv', **kw))
        self.box_head = BoxHead(HeadLayer.linear(*p[BOX_KEYS[0]], relu=True, **kw), HeadLayer.linear(*p[BOX_KEYS[1]], relu=True, **kw),
                                HeadLayer.siblings(p[BOX_KEYS[2]], p[BOX_KEYS[3]], 'linear', **kw))
        self.mask_head = None
        if MASK_KEYS[0] in p:
            self.mask_head = MaskHead([HeadLayer.conv(*p[k], relu=True, **kw) for k in MASK_KEYS[:4]], HeadLayer.deconv(*p[MASK_KEYS[4]], relu=True, **kw),
                                      HeadLayer.conv(*p[MASK_KEYS[5]], relu=False, **kw))

    def _init_trainable(self, p, dtype, device):
        """DESIGN.md section 28.  The parameters live on the device in torchvision's layout under torchvision's names (parameters(),
        named_parameters(), state_dict(), load_state_dict(): a checkpoint's head keys go in and out as they are; torch.optim works on them).
        Forward and backward read packings made on the device (cosy_head_weight_pack) when a parameter's _version has moved; pack_count counts
        those launches.  rpn_head / box_head / mask_head are one autograd node each when grad is enabled and an input or a parameter requires
        grad, and exactly the inference path otherwise.  With train_dtype=torch.bfloat16 (section 32) the rows a node keeps, the gradient rows
        and both packings are bfloat16 under the float32 parameters, the master weights; the forward is that of bfloat16 inference heads."""
        if dtype != torch.float32:
            raise ValueError(f'trainable heads are float32 only (16-bit training and master weights are not built), got dtype={dtype}')
        if device is None:
            w = p[RPN_KEYS[0]][0]
            device = w.device if torch.is_tensor(w) and w.is_cuda else None
        self._counter = [0]
        kw = dict(device=device, counter=self._counter, dtype=self.train_dtype)
        T = TrainableLayer
        self.rpn_head = RpnHead(T.conv(*p[RPN_KEYS[0]], relu=True, **kw), T.siblings(p[RPN_KEYS[1]], p[RPN_KEYS[2]], 'conv', **kw))
        self.box_head = BoxHead(T.linear(*p[BOX_KEYS[0]], relu=True, **kw), T.linear(*p[BOX_KEYS[1]], relu=True, **kw),
                                T.siblings(p[BOX_KEYS[2]], p[BOX_KEYS[3]], 'linear', **kw))
        self.mask_head = None
        named = [(RPN_KEYS[0], self.rpn_head.conv.pairs[0]), (RPN_KEYS[1], self.rpn_head.pred.pairs[0]), (RPN_KEYS[2], self.rpn_head.pred.pairs[1]),
                 (BOX_KEYS[0], self.box_head.fc6.pairs[0]), (BOX_KEYS[1], self.box_head.fc7.pairs[0]), (BOX_KEYS[2], self.box_head.pred.pairs[0]),
                 (BOX_KEYS[3], self.box_head.pred.pairs[1])]
        if MASK_KEYS[0] in p:
            self.mask_head = MaskHead([T.conv(*p[k], relu=True, **kw) for k in MASK_KEYS[:4]], T.deconv(*p[MASK_KEYS[4]], relu=True, **kw),
                                      T.conv(*p[MASK_KEYS[5]], relu=False, **kw))
            named += [(k, layer.pairs[0]) for k, layer in zip(MASK_KEYS, self.mask_head.convs + [self.mask_head.deconv, self.mask_head.logits])]
        self._named = [(f'{k}.{part}', t) for k, pair in named for part, t in zip(('weight', 'bias'), pair)]

    @property
    def pack_count(self):
        """device weight packs launched so far (trainable heads): one per layer whose parameters moved since its last pack"""
        return self._counter[0]

    def _need_trainable(self, what):
        if not self.trainable:
            raise RuntimeError(f'{what}: these DetectorHeads are inference only; build them with trainable=True')

    def named_parameters(self):
        self._need_trainable('named_parameters')
        return list(self._named)

    def parameters(self):
        self._need_trainable('parameters')
        return [t for _, t in self._named]

    def state_dict(self):
        """{torchvision's key: a detached copy of the parameter}"""
        self._need_trainable('state_dict')
        return {k: t.detach().clone() for k, t in self._named}

    def load_state_dict(self, sd, strict=True):
        """copies a Mask R-CNN state_dict's head keys into the parameters (in place: their _version moves, the next forward packs again); the
        trunk's and the FPN's keys are ignored, a missing head key is a KeyError naming it (strict) or is left as it is"""
        self._need_trainable('load_state_dict')
        for k, t in self._named:
            if k not in sd:
                if strict:
                    raise KeyError(k)
                continue
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f'{k} must be {tuple(t.shape)}, got {tuple(sd[k].shape)}')
            with torch.no_grad():
                t.copy_(sd[k])

    def zero_grad(self):
        for t in self.parameters():
            t.grad = None

    def layers(self):
        """every packed layer, in a fixed order (tests compare their bytes)"""
        out = [self.rpn_head.conv, self.rpn_head.pred, self.box_head.fc6, self.box_head.fc7, self.box_head.pred]
        if self.mask_head is not None:
            out += self.mask_head.convs + [self.mask_head.deconv, self.mask_head.logits]
        return out

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float32, device=None, trainable=False, train_dtype=None):
        """a Mask R-CNN state_dict as it is: the trunk's and the FPN's keys are ignored, a missing head key is a KeyError naming it.
        dtype stays the type of the parameters; train_dtype names the rows of trainable heads (see __init__)"""
        if trainable and dtype != torch.float32:
            raise ValueError(f'trainable heads are float32 only (16-bit training and master weights are not built), got dtype={dtype}')
        params = {}
        for k in RPN_KEYS + BOX_KEYS + MASK_KEYS:
            for part in ('weight', 'bias'):
                if f'{k}.{part}' not in sd:
                    raise KeyError(f'{k}.{part}')
            params[k] = (sd[f'{k}.weight'], sd[f'{k}.bias'])
        return cls(params, dtype, device, trainable, train_dtype)

    @classmethod
    def from_modules(cls, rpn_head, box_head, box_predictor, mask_head=None, mask_predictor=None, dtype=torch.float32, device=None, trainable=False,
                     train_dtype=None):
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
        if trainable:           # parameters of the heads' own: a copy, never the modules' tensors
            params = {k: tuple(None if t is None else t.detach().clone() for t in pair) for k, pair in params.items()}
        return cls(params, dtype, device, trainable, train_dtype)

"""The backward of the detector's trunk on the matrix pipe: the data and weight gradients of the ResNet
bottlenecks and the FPN as GEMMs (HIP: csrc/kernels_detbwd.hip, the heads' gradient kernels -- cosy_trunk_weight_pack, cosy_trunk_dgrad, cosy_trunk_wgrad), the
trainable layer that holds a trunk parameter, and the autograd node behind DetectorTrunk(trainable=True).  float32, or with
train_dtype=torch.bfloat16 (section 30; the same entry points with `16` appended, picked by _lib.rows_entry, and cosy_trunk_grad_pack16)
bfloat16 rows and packed weights under float32 parameters, the master weights, and float32 gradients.

A trunk layer is v = fmaf(conv_stride(x, W), scale, shift) [+ r], y = relu(v).  Its gradient rows g are the gradient at v, float32 rows on
the layer's OUTPUT grid.  No scaled copy of g is stored: the data gradient reads ws = w scale[o] (packed once per weight version), the weight
gradient multiplies by scale[o] in its second pass.  The store of a data-gradient launch adds the shortcut's and the FPN's contributions and
applies the ReLU mask of the block below: no element-wise launch sits between two GEMMs.
"""
import contextlib
import ctypes

import torch

from . import _lib
from .detector_heads import MAX_ROWS, PackedOnDevice, _describe, _g, _grad_pack, _gemm, _wgrad_buffers

F32, BF16 = torch.float32, torch.bfloat16
SAME, EVEN, NEAREST_T = _lib.TRUNK_ADD_SAME, _lib.TRUNK_ADD_EVEN, _lib.TRUNK_ADD_NEAREST_T


def _out(n, stride):
    return (n - 1) // stride + 1


def check_train_dtype(trainable, train_dtype, owner='trunk'):
    """the train_dtype= keyword of the trainable trunk, heads and detector -> the type of the rows and of the packed weights (None: not trainable)"""
    if train_dtype is None:
        return F32 if trainable else None
    if not trainable:
        raise ValueError(f'train_dtype={train_dtype} names the rows of a trainable {owner}: give trainable=True with it')
    if train_dtype == torch.float16:
        raise ValueError('train_dtype=torch.float16: float16 training needs a loss scaler, which is not built; use torch.bfloat16 or torch.float32')
    if train_dtype not in (F32, BF16):
        raise ValueError(f'train_dtype must be None, torch.float32 or torch.bfloat16, got {train_dtype!r}')
    return train_dtype


class TrainableTrunkLayer(PackedOnDevice):
    """A trainable convolution of the trunk: weight is a torch.nn.Parameter (O,C,k,k) on the device under torchvision's name; a layer followed
    by FrozenBatchNorm keeps its scale and shift as constants, an FPN layer has a bias Parameter and no scale.  w / bias (what cosy_trunk_conv
    and cosy_head_conv read, the host packing's bytes) and w_t (the transposed, tap-flipped packing of ws = w scale[o]) are written by
    cosy_trunk_weight_pack when a parameter's _version or storage has moved since the last pack.  dtype: the type of the rows and of w / w_t
    (the parameters are float32 whatever it is); torch.bfloat16 packs through cosy_trunk_weight_pack16: w holds the bytes of the host packing of
    the weight rounded to bfloat16, w_t those of ws rounded once."""
    kind, dtype, owner = 'conv', F32, 'trunk'

    def __init__(self, name, weight, bn=None, bias=None, stride=1, relu=False, device=None, counter=None, dtype=F32):
        from .detector_trunk import frozen_bn
        if device is None or torch.device(device).type != 'cuda':
            raise ValueError(f'{name}: a trainable trunk lives on the ROCm device: give device=, got {device}')
        if not torch.is_tensor(weight) or weight.dim() != 4:
            raise ValueError(f'{name}.weight must be a 4-d tensor')
        O, C, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        if weight.shape[3] != k or k not in (1, 3):
            raise ValueError(f'{name}: a trainable trunk convolution is 1x1 or 3x3, got a weight of {tuple(weight.shape)}')
        if stride not in (1, 2):
            raise ValueError(f'{name}: stride must be 1 or 2, got {stride}')
        if C % 8 or O % 8:
            raise ValueError(f'{name}: {C} -> {O} channels: every channel count must be a multiple of 8')
        if dtype not in (F32, BF16):
            raise ValueError(f'{name}: the rows of a trainable trunk are float32 or bfloat16, got {dtype}')
        self.dtype = dtype
        self.name, self.ksize, self.stride, self.relu = name, k, int(stride), bool(relu)
        self.c_in, self.c_out, self.n_out = C, O, O
        self.counter = counter if counter is not None else [0]
        self.weight = torch.nn.Parameter(weight.detach().to(device=device, dtype=F32).contiguous().clone())
        self.device = dev = self.weight.device
        NP = -(-O // 64) * 64
        self.bias_param, self.scale, self.shift = None, None, None
        if bn is not None:
            scale, shift = frozen_bn(*bn)
            if scale.shape[0] != O:
                raise ValueError(f'{name}: the batch norm holds {scale.shape[0]} channels, the convolution {O}')
            self.scale = torch.zeros(NP, dtype=F32)
            self.scale[:O] = scale
            self.scale, self.shift = self.scale.to(dev), shift.to(dev).contiguous()
        else:
            b = torch.zeros(O) if bias is None else bias
            if b.dim() != 1 or b.shape[0] != O:
                raise ValueError(f'{name}.bias must be ({O}), got {tuple(b.shape)}')
            self.bias_param = torch.nn.Parameter(b.detach().to(device=dev, dtype=F32).contiguous().clone())
        self._alloc_packings()

    def parameters(self):
        return [self.weight] + ([self.bias_param] if self.bias_param is not None else [])

    def pack_args(self):
        return self.weight, (self.shift if self.bias_param is None else self.bias_param), None, None, self.scale, self.ksize, self.c_in, self.c_out, 0

    def _pack(self):
        w, shift, _, _, scale, ksize, c_in, c_out, _ = self.pack_args()
        _lib.check(_lib.rows_entry('cosy_trunk_weight_pack', self.dtype)(_lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), ksize, c_in, c_out, _lib.ptr(self.w),
                                                                       _lib.ptr(self.bias), _lib.ptr(self.w_t), _lib.stream()))

    ready = PackedOnDevice.refresh

    def out_size(self, H, W):
        return _out(H, self.stride), _out(W, self.stride)


# ---- launches ------------------------------------------------------------------------------------------------------------------------
def trunk_dgrad(layer, g_rows, B, H, W, out, adds=(), y=None, store=_lib.HEAD_STORE_ROWS, stride=None):
    """one cosy_trunk_dgrad call: g_rows on the layer's output grid -> dX on B maps of H x W cells.  adds: up to two (rule, rows, H, W);
    y: the mask rows on the dX grid.  stride: the layer's own unless given (downsample.0 runs at stride 1 on its output grid)"""
    d = _lib.HeadLayer()
    d.x, d.w, d.out = _lib.ptr(g_rows), _lib.ptr(layer.w_t), _lib.ptr(out)
    d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split = _lib.DTYPES[layer.dtype], layer.ksize, layer.c_out, layer.c_in, 0, store, layer.c_in
    _describe(d, [(B, H, W)])
    adds = list(adds)
    if len(adds) > 2:
        raise ValueError(f'a data-gradient store takes at most two add operands, got {len(adds)}')
    flat = []
    for rule, rows, aH, aW in adds + [(_lib.TRUNK_ADD_NONE, None, 0, 0)] * (2 - len(adds)):
        flat += [_lib.ptr(rows), rule, aH, aW]
    dgrad = _lib.rows_entry('cosy_trunk_dgrad', layer.dtype)
    _lib.check(dgrad(ctypes.byref(d), layer.stride if stride is None else stride, *flat, _lib.ptr(y), _lib.stream()))
    return out


def trunk_wgrad(layer, x_rows, g_rows, B, H, W):
    """one cosy_trunk_wgrad call: x_rows on B maps of H x W cells, g_rows on the output grid -> [dW (, db)] in the parameters' layout"""
    d = _lib.HeadLayer()
    d.x = _lib.ptr(x_rows)
    d.dtype, d.ksize, d.c_in, d.c_out, d.n_split = _lib.DTYPES[layer.dtype], layer.ksize, layer.c_in, layer.c_out, layer.c_out
    _describe(d, [(B, H, W)])
    Ho, Wo = layer.out_size(H, W)
    out, ws, need = _wgrad_buffers(layer, B * Ho * Wo, layer.ksize, layer.c_out)
    wgrad = _lib.rows_entry('cosy_trunk_wgrad', layer.dtype)
    _lib.check(wgrad(ctypes.byref(d), layer.stride, _lib.ptr(g_rows), _lib.ptr(layer.scale), _lib.ptr(out[0]), _lib.ptr(out[1]) if len(out) > 1 else None,
                     _lib.ptr(ws), need, _lib.stream()))
    return out


def trunk_grad_pack(g, rows, B, C, HW):
    """the NCHW float32 gradient of one map (None: zeros) -> the rows (B HW, C) of the rows' type, one launch"""
    if rows.dtype == F32:
        return _grad_pack(g, None, rows, B, C, 0, HW)
    if g is not None and (g.dtype != F32 or g.numel() != B * C * HW or not g.is_cuda):
        raise ValueError(f'a gradient of {B} x {C} x {HW} float32 values on the device was expected, got {tuple(g.shape)} {g.dtype} on {g.device}')
    if B:
        _lib.check(_lib.rows_entry('cosy_trunk_grad_pack', rows.dtype)(_lib.ptr(None if g is None else g.contiguous()), _lib.ptr(rows), B, C, HW, _lib.stream()))
    return rows


def _rows_of(t, dtype):
    """(B,C,H,W) -> rows (B H W, C) of dtype (the tests' access: a bfloat16 layer rounds its operands to nearest even on the way in)"""
    return t.detach().permute(0, 2, 3, 1).contiguous().view(-1, int(t.shape[1])).to(dtype)


def layer_dgrad(layer, grad, H, W, adds=(), y=None, stride=None):
    """One layer's data gradient through the kernel, NCHW in and out (the tests' access).  grad (B,O,Ho,Wo) float32 at the layer's pre-activation
    output; H, W: the dX grid; adds: (rule, (B,C,h,w) float32 map); y: (B,C,H,W) float32, the stored output of the layer below -> (B,C,H,W)"""
    dev = grad.device
    layer.ready(dev)
    B, O, Ho, Wo = (int(v) for v in grad.shape)
    rows = lambda t: _rows_of(t, layer.dtype)
    ops = [(rule, rows(t), int(t.shape[2]), int(t.shape[3])) for rule, t in adds]
    with torch.cuda.device(dev):
        if layer.dtype != F32:                                  # 16-bit rows have the row store alone; the way out is exact
            out = torch.empty((B * H * W, layer.c_in), dtype=layer.dtype, device=dev)
            trunk_dgrad(layer, rows(grad), B, H, W, out, ops, None if y is None else rows(y), _lib.HEAD_STORE_ROWS, stride)
            return out.view(B, H, W, layer.c_in).permute(0, 3, 1, 2).float().contiguous()
        out = torch.empty((B, layer.c_in, H, W), dtype=F32, device=dev)
        trunk_dgrad(layer, rows(grad), B, H, W, out, ops, None if y is None else rows(y), _lib.HEAD_STORE_NCHW, stride)
    return out


def layer_wgrad(layer, x, grad):
    """One layer's weight gradient through the kernel: x (B,C,H,W), grad (B,O,Ho,Wo) float32 -> [dW (, db)]"""
    dev = x.device
    layer.ready(dev)
    B, C, H, W = (int(v) for v in x.shape)
    with torch.cuda.device(dev):
        return trunk_wgrad(layer, _rows_of(x, layer.dtype), _rows_of(grad, layer.dtype), B, H, W)


# ---- the node --------------------------------------------------------------------------------------------------------------------------
def forward_keep(trunk, images):
    """section 27's launches; the stages below train_from_stage and the stem run in the trunk's arena and keep nothing, the rows the backward
    reads (x, a, b, out of every trainable block, the stage outputs, the laterals) are tensors of their own -> the four maps, keep"""
    from .detector_trunk import _trunk_gemm
    dev, B = images.device, int(images.shape[0])
    fresh = lambda n, c: torch.empty((n, c), dtype=trunk.dtype, device=dev)            # the rows' type: float32, or section 30's bfloat16
    x, H, W = trunk.stem_rows(images)
    tfs = trunk.train_from_stage
    if tfs == 1:
        x = x.clone()
    blocks_keep, feats, flip = {}, [], 0
    for si, blocks in enumerate(trunk.stages):
        for bi, blk in enumerate(blocks):
            stage_out = f'stage{si}'
            name = stage_out if bi == len(blocks) - 1 else f'x{flip}'
            if si + 1 >= tfs:
                kept = {}

                def buf(slot, n, c, kept=kept):
                    kept[slot] = fresh(n, c)
                    return kept[slot]
                out, Ho, Wo = blk.rows(x, B, H, W, buf, name)
                blocks_keep[(si + 1, bi)] = dict(x=x, a=kept['a'], b=kept['b'], out=out, H=H, W=W, Ho=Ho, Wo=Wo)
            else:
                out, Ho, Wo = blk.rows(x, B, H, W, lambda slot, n, c: fresh(n, c) if slot == stage_out else trunk._buf(slot, n, c), name)
            x, H, W = out, Ho, Wo
            flip ^= 1
        feats.append((x, H, W))
    L, C = len(feats), trunk.outer[0].c_out
    starts = [0]
    for _, h, w in feats:
        starts.append(starts[-1] + B * h * w)
    if starts[-1] > MAX_ROWS:
        raise ValueError(f'{starts[-1]} rows (cells of all levels) exceed the limit of 2^30 per launch')
    inner = fresh(starts[-1], trunk.inner[0].c_out)
    for l in range(L - 1, -1, -1):
        rows, h, w = feats[l]
        res, res_hw = (None, None) if l == L - 1 else (inner[starts[l + 1]:starts[l + 2]], feats[l + 1][1:])
        _trunk_gemm(trunk.inner[l], rows, B, h, w, inner[starts[l]:starts[l + 1]], residual=res, res_hw=res_hw)
    flat = torch.empty(C * starts[-1], dtype=F32, device=dev)
    for l, (_, h, w) in enumerate(feats):
        _gemm(trunk.outer[l], inner[starts[l]:starts[l + 1]], [(B, h, w)], _lib.HEAD_STORE_NCHW, flat[C * starts[l]:C * starts[l + 1]])
    out = [flat[C * starts[l]:C * starts[l + 1]].view(B, C, h, w) for l, (_, h, w) in enumerate(feats)]
    return out, dict(blocks=blocks_keep, feats=feats, inner=inner, starts=starts, B=B)


def kept_bytes(keep):
    """bytes of the rows a forward holds for its backward"""
    seen, total = set(), 0
    tensors = [keep['inner']] + [f[0] for f in keep['feats']] + [t for k in keep['blocks'].values() for t in (k['x'], k['a'], k['b'], k['out'])]
    for t in tensors:
        key = t.untyped_storage().data_ptr() if hasattr(t, 'untyped_storage') else t.data_ptr()
        if key not in seen:
            seen.add(key)
            total += t.numel() * t.element_size()
    return total


def backward(trunk, keep, grads, rows_out=None, timer=None):
    """section 29's chain.  grads: the NCHW gradients at the four maps (None: zeros).  -> {id(parameter): gradient}.  rows_out: a dict that
    receives every gradient row buffer under the twin's names (the tests).  timer: a callable (group) -> context manager ('fpn', 'dgrad', 'wgrad')"""
    B, feats, inner, starts, bk = keep['B'], keep['feats'], keep['inner'], keep['starts'], keep['blocks']
    dev = inner.device
    L, tfs = len(trunk.stages), trunk.train_from_stage
    new = lambda n, c: torch.empty((n, c), dtype=trunk.dtype, device=dev)
    timed = timer if timer is not None else (lambda group: contextlib.nullcontext())
    out = {}

    def note(name, rows, h, w):
        if rows_out is not None:
            rows_out[name] = (rows, B, h, w)

    def put(layer, grads_):
        for p, g in zip(layer.parameters(), grads_):
            out[id(p)] = g
    C = trunk.outer[0].c_out
    G = []
    with timed('fpn'):
        for l in range(L):
            _, h, w = feats[l]
            g = trunk_grad_pack(_g(grads[l]), new(B * h * w, C), B, C, h * w)
            x_in = inner[starts[l]:starts[l + 1]]
            put(trunk.outer[l], trunk_wgrad(trunk.outer[l], x_in, g, B, h, w))
            adds = [] if l == 0 else [(NEAREST_T, G[l - 1], feats[l - 1][1], feats[l - 1][2])]
            G.append(trunk_dgrad(trunk.outer[l], g, B, h, w, new(B * h * w, trunk.inner[l].c_out), adds))
            note(f'fpn.G_inner.{l}', G[l], h, w)
            put(trunk.inner[l], trunk_wgrad(trunk.inner[l], feats[l][0], G[l], B, h, w))

    def lateral(s, masked):
        rows, h, w = feats[s - 1]
        with timed('fpn'):
            r = trunk_dgrad(trunk.inner[s - 1], G[s - 1], B, h, w, new(B * h * w, trunk.inner[s - 1].c_in), y=rows if masked else None)
        note(f'fpn.lateral_dx.{s - 1}', r, h, w)
        return r
    g3 = None
    for s in range(L, tfs - 1, -1):
        blocks = trunk.stages[s - 1]
        if s == L:
            g3 = lateral(s, True)
        for i in range(len(blocks) - 1, -1, -1):
            blk, k = blocks[i], bk[(s, i)]
            H, W, Ho, Wo = k['H'], k['W'], k['Ho'], k['Wo']
            name = f'body.layer{s}.{i}'
            first = s == tfs and i == 0
            with timed('dgrad'):
                g2 = trunk_dgrad(blk.conv3, g3, B, Ho, Wo, new(B * Ho * Wo, blk.conv3.c_in), y=k['b'])
                g1 = trunk_dgrad(blk.conv2, g2, B, H, W, new(B * H * W, blk.conv2.c_in), y=k['a'])
            note(f'{name}.g3', g3, Ho, Wo), note(f'{name}.g2', g2, Ho, Wo), note(f'{name}.g1', g1, H, W)
            with timed('wgrad'):
                put(blk.conv3, trunk_wgrad(blk.conv3, k['b'], g3, B, Ho, Wo))
                put(blk.conv2, trunk_wgrad(blk.conv2, k['a'], g2, B, H, W))
                put(blk.conv1, trunk_wgrad(blk.conv1, k['x'], g1, B, H, W))
                if blk.downsample is not None:
                    put(blk.downsample, trunk_wgrad(blk.downsample, k['x'], g3, B, H, W))
            if first:
                break
            tail = [(SAME, lateral(s - 1, False), H, W)] if i == 0 else []
            with timed('dgrad'):
                if blk.downsample is None:
                    adds = [(SAME, g3, H, W)]
                else:
                    d = trunk_dgrad(blk.downsample, g3, B, Ho, Wo, new(B * Ho * Wo, blk.downsample.c_in), stride=1)
                    note(f'{name}.down_dx', d, Ho, Wo)
                    adds = [(EVEN if blk.conv2.stride == 2 else SAME, d, Ho, Wo)]
                g3 = trunk_dgrad(blk.conv1, g1, B, H, W, new(B * H * W, blk.conv1.c_in), adds + tail, y=k['x'])
    return out


class TrunkFn(torch.autograd.Function):
    """trunk(images) as one node: forward = section 27's launches, backward = section 29's"""

    @staticmethod
    def forward(ctx, trunk, images, *params):
        out, keep = forward_keep(trunk, images)
        ctx.trunk, ctx.keep, ctx.n = trunk, keep, len(params)
        trunk.last_kept_bytes = kept_bytes(keep)
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError('DetectorTrunk: double backward is not built (the backward of the trunk\'s backward has no kernel); '
                               'call backward() without create_graph')
        trunk = ctx.trunk
        rows_out = {} if trunk.keep_rows else None
        with torch.cuda.device(ctx.keep['inner'].device):
            got = backward(trunk, ctx.keep, grads, rows_out, trunk.timer)
        if rows_out is not None:
            trunk.last_rows = rows_out
        return (None, None) + tuple(got.get(id(p)) for p in trunk.parameters())

"""The detector's trunk on the matrix pipe: torchvision 0.4.2's ResNet-50 body with FrozenBatchNorm2d and its FeaturePyramidNetwork, the part
of Mask R-CNN between detector_input and DetectorHeads, and `Detector`, the reference's interface over the whole chain.  Inference only by
default; trainable=True makes the trunk an autograd node with float32 parameters (detector_trunk_backward.py), on
float32 rows or with train_dtype=torch.bfloat16 on bfloat16 rows and packed weights (section 30).
DESIGN.md section 27 states the contract; HIP: csrc/kernels_dettrunk.hip (cosy_trunk_conv, cosy_trunk_stem_pack, cosy_trunk_maxpool) and the
GEMM it shares with the heads (csrc/dethead_device.h).

Every convolution is the heads' implicit GEMM over rows (detector_heads.py) with a stride of 1 or 2 and the epilogue
fmaf(acc, scale, shift) -> + residual -> ReLU -> store: FrozenBatchNorm is the scale and shift, a bottleneck's shortcut and the FPN's
nearest-upsampled coarser level are the residual.  Between the layers the activations are rows in the storage type, in an arena the trunk
owns and reuses from call to call (so one trunk serves one stream at a time); the five maps leave as contiguous NCHW float32.
Launches for ResNet-50 + FPN: stem pack, stem GEMM, pool, 52 GEMMs of the body, 4 lateral GEMMs, 4 output GEMMs (cosy_head_conv: every level
has weights of its own) into one flat buffer.
"""
import ctypes
import re

import torch

from . import _lib
from .detector_heads import HeadLayer, _check_input, _describe, _dtype, _gemm, _pack, _ready, MAX_ROWS

_DTYPES = _lib.DTYPES
STEM_ROW = 152                                # 7 x 7 x 3 = 147 taps x channels of the stem, padded to a multiple of 8
LEVELS = ('0', '1', '2', '3', 'pool')
_BN = ('weight', 'bias', 'running_mean', 'running_var')


def frozen_bn(weight, bias, running_mean, running_var):
    """FrozenBatchNorm2d of torchvision 0.4.2 (no eps) -> scale, shift: float32, on the CPU"""
    w, b, m, v = (t.detach().to(device='cpu', dtype=torch.float32) for t in (weight, bias, running_mean, running_var))
    scale = w * v.rsqrt()
    return scale, b - m * scale


class TrunkLayer(HeadLayer):
    """one packed convolution of the trunk: a HeadLayer (its bias is the shift) with a stride and, for a conv followed by FrozenBatchNorm, the
    per-channel scale, float32 whatever the storage type and padded like the bias.  kind 'conv' (ksize 1 or 3) or 'stem' (the 7x7 stride-2
    convolution as a one-tap GEMM over cosy_trunk_stem_pack's rows of 152)"""

    def __init__(self, name, weight, bn=None, bias=None, stride=1, relu=False, dtype=torch.float32, device=None):
        w = self._f32(weight, f'{name}.weight', 4)
        O, C, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        stem = k == 7
        if w.shape[3] != k or k not in (1, 3, 7) or (stem and C != 3):
            raise ValueError(f'{name}: a trunk convolution is 1x1, 3x3, or the 7x7 stem over 3 channels, got a weight of {tuple(w.shape)}')
        if stride not in (1, 2) or (stem and stride != 2):
            raise ValueError(f'{name}: stride must be 1 or 2 (the stem: 2), got {stride}')
        if not stem and C % 8:
            raise ValueError(f'{name}: {C} input channels: every channel count but the image\'s 3 must be a multiple of 8')
        if stem:
            rows = torch.zeros((O, 1, STEM_ROW), dtype=torch.float32)
            rows[:, 0, :147] = w.permute(0, 2, 3, 1).reshape(O, 147)                 # element (ky 7 + kx) 3 + c
        else:
            rows = w.permute(0, 2, 3, 1).reshape(O, k * k, C)
        if bn is not None:
            scale, shift = frozen_bn(*bn)
            if scale.shape[0] != O:
                raise ValueError(f'{name}: the batch norm holds {scale.shape[0]} channels, the convolution {O}')
        else:
            scale, shift = None, self._bias(bias, O, f'{name}.bias')
        super().__init__('stem' if stem else 'conv', rows, shift, 1 if stem else k, relu, dtype, device)
        self.name, self.stride = name, 1 if stem else int(stride)
        self.packed_scale = None
        if scale is not None:
            self.packed_scale = torch.zeros_like(self.packed_bias)
            self.packed_scale[:O] = scale
        self.scale = self.packed_scale.to(self.device) if scale is not None and self.device is not None else None

    def ready(self, dev):
        """detector_heads._ready, and the scale beside the weights"""
        _ready(self, dev)
        if self.packed_scale is not None and self.scale is None:
            self.scale = self.packed_scale.to(dev)
        return self

    def out_size(self, H, W):
        return (H - 1) // self.stride + 1, (W - 1) // self.stride + 1


def _out2(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _trunk_gemm(layer, x_rows, B, H, W, out, store=_lib.HEAD_STORE_ROWS, residual=None, res_hw=None):
    """one cosy_trunk_conv launch over B maps of H x W input cells; residual: rows on maps of res_hw per image"""
    d = _lib.HeadLayer()
    d.x, d.w, d.bias, d.out, d.out1 = _lib.ptr(x_rows), _lib.ptr(layer.w), _lib.ptr(layer.bias), _lib.ptr(out), None
    d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store = _DTYPES[layer.dtype], layer.ksize, layer.c_in, layer.c_out, int(layer.relu), store
    d.n_split = layer.c_out
    _describe(d, [(B, H, W)])
    rh, rw = res_hw if residual is not None else (0, 0)
    if B:
        _lib.check(_lib.lib().cosy_trunk_conv(ctypes.byref(d), layer.stride, _lib.ptr(layer.scale), _lib.ptr(residual), rh, rw, _lib.stream()))
    return out


def _input(x, name, channels):
    x = _check_input(x, name, 4, channels, '(B,C,H,W)')
    if not x.is_cuda:
        raise ValueError(f'{name} must live on the ROCm device (got a CPU tensor); there is no CPU fallback')
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError(f'{name} requires grad: DetectorTrunk is inference only, training keeps the torch.nn modules and autograd '
                           '(detector_train.detector_losses); call it under torch.no_grad() or detach the input')
    if x.shape[0] and (x.shape[2] < 1 or x.shape[3] < 1):
        raise ValueError(f'{name} must have at least one cell, got {tuple(x.shape)}')
    return x.contiguous()


def _to_rows(x, dtype):
    """contiguous NCHW float32 -> rows of the storage type"""
    B, C, H, W = (int(v) for v in x.shape)
    rows = torch.empty((B * H * W, C), dtype=dtype, device=x.device)
    _pack(x, rows, B, C, H * W, dtype)
    return rows


def _to_nchw(rows, B, H, W):
    """rows of the storage type -> NCHW float32 (the access functions' way out; the trunk itself stores NCHW from the GEMM)"""
    return rows.view(B, H, W, int(rows.shape[1])).permute(0, 3, 1, 2).float().contiguous()


def trunk_conv_layer(x, layer, residual=None, store='nchw'):
    """One layer through cosy_trunk_conv.  x (B,C,H,W) float32 on the device (the stem: (B,3,H,W) images), rounded to the layer's storage type
    on the way in; residual: (B,N,rH,rW) float32, rounded likewise, added by the nearest rule.  -> (B,N,Ho,Wo) float32, or with store='rows'
    the rows (B Ho Wo, N) of the storage type."""
    if not isinstance(layer, TrunkLayer):
        raise ValueError(f'layer must be a TrunkLayer, got {type(layer).__name__}')
    if store not in ('nchw', 'rows'):
        raise ValueError(f"store must be 'nchw' or 'rows', got {store!r}")
    x = _input(x, 'x', 3 if layer.kind == 'stem' else layer.c_in)
    dev = x.device
    layer.ready(dev)
    B, _, H, W = (int(v) for v in x.shape)
    if layer.kind == 'stem':
        H, W = _out2(H, W)
        rows = torch.empty((B * H * W, STEM_ROW), dtype=layer.dtype, device=dev)
        if B:
            _lib.check(_lib.lib().cosy_trunk_stem_pack(_lib.ptr(x), _lib.ptr(rows), B, int(x.shape[2]), int(x.shape[3]), _DTYPES[layer.dtype], _lib.stream()))
    else:
        rows = _to_rows(x, layer.dtype)
    Ho, Wo = layer.out_size(H, W)
    res, res_hw = None, None
    if residual is not None:
        residual = _input(residual, 'residual', layer.c_out)
        if int(residual.shape[0]) != B:
            raise ValueError(f'residual must hold the {B} images of x, got {tuple(residual.shape)}')
        res, res_hw = _to_rows(residual, layer.dtype), (int(residual.shape[2]), int(residual.shape[3]))
    if store == 'rows':
        return _trunk_gemm(layer, rows, B, H, W, torch.empty((B * Ho * Wo, layer.c_out), dtype=layer.dtype, device=dev), _lib.HEAD_STORE_ROWS, res, res_hw)
    return _trunk_gemm(layer, rows, B, H, W, torch.empty((B, layer.c_out, Ho, Wo), dtype=torch.float32, device=dev), _lib.HEAD_STORE_NCHW, res, res_hw)


def max_pool_rows(x_rows, B, H, W, out=None):
    """rows (B H W, C) -> rows (B Ho Wo, C): max_pool2d(3, 2, 1) with torch's -inf padding and NaN rule"""
    C = int(x_rows.shape[1])
    Ho, Wo = _out2(H, W)
    if out is None:
        out = torch.empty((B * Ho * Wo, C), dtype=x_rows.dtype, device=x_rows.device)
    if B:
        _lib.check(_lib.lib().cosy_trunk_maxpool(_lib.ptr(x_rows), _lib.ptr(out), B, H, W, C, _DTYPES[x_rows.dtype], _lib.stream()))
    return out


def max_pool(x, dtype=torch.float32):
    """(B,C,H,W) float32 -> (B,C,Ho,Wo) float32 through the rows kernel in the storage type `dtype`"""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] < 8 or x.shape[1] % 8:
        raise ValueError(f'x must be (B,C,H,W) with a positive multiple of 8 channels, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    x = _input(x, 'x', int(x.shape[1]))
    B, C, H, W = (int(v) for v in x.shape)
    return _to_nchw(max_pool_rows(_to_rows(x, _dtype(dtype)), B, H, W), B, *_out2(H, W))


class Bottleneck:
    """conv1 (1x1) -> conv2 (3x3, carries the stride) -> conv3 (1x1) with the shortcut (the input, or downsample(input)) and the ReLU in its
    epilogue.  Called with rows by the trunk; trunk.block(stage, i)(x_nchw) is the access the tests use."""

    def __init__(self, conv1, conv2, conv3, downsample=None):
        self.conv1, self.conv2, self.conv3, self.downsample = conv1, conv2, conv3, downsample
        if conv2.c_in != conv1.c_out or conv3.c_in != conv2.c_out:
            raise ValueError(f'{conv1.name}: the bottleneck\'s widths do not chain')
        if downsample is None and (conv3.c_out != conv1.c_in or conv2.stride != 1):
            raise ValueError(f'{conv1.name}: a bottleneck that changes the width or the size needs a downsample')
        if downsample is not None and (downsample.c_in != conv1.c_in or downsample.c_out != conv3.c_out or downsample.stride != conv2.stride):
            raise ValueError(f'{downsample.name}: {downsample.c_in} -> {downsample.c_out} stride {downsample.stride} does not match the block')

    def layers(self):
        return [self.conv1, self.conv2, self.conv3] + ([self.downsample] if self.downsample is not None else [])

    def rows(self, x, B, H, W, buf, out_name):
        """x: rows (B H W, c_in) -> rows (B Ho Wo, c_out) in the slot out_name of buf(name, rows, channels)"""
        Ho, Wo = self.conv2.out_size(H, W)
        a = _trunk_gemm(self.conv1, x, B, H, W, buf('a', B * H * W, self.conv1.c_out))
        b = _trunk_gemm(self.conv2, a, B, H, W, buf('b', B * Ho * Wo, self.conv2.c_out))
        short = x
        if self.downsample is not None:
            short = _trunk_gemm(self.downsample, x, B, H, W, buf('down', B * Ho * Wo, self.downsample.c_out))
        return _trunk_gemm(self.conv3, b, B, Ho, Wo, buf(out_name, B * Ho * Wo, self.conv3.c_out), residual=short, res_hw=(Ho, Wo)), Ho, Wo

    def __call__(self, x):
        x = _input(x, 'x', self.conv1.c_in)
        dev, dtype = x.device, self.conv1.dtype
        for layer in self.layers():
            layer.ready(dev)
        B, _, H, W = (int(v) for v in x.shape)
        out, Ho, Wo = self.rows(_to_rows(x, dtype), B, H, W, lambda name, n, c: torch.empty((n, c), dtype=dtype, device=dev), 'out')
        return _to_nchw(out, B, Ho, Wo)


class DetectorTrunk:
    """trunk(images (B,3,H,W) float32) -> the five contiguous NCHW float32 maps ['0', '1', '2', '3', 'pool']: the backbone(images) contract of
    detections_from_frames.  Built from a state dict (from_state_dict) or a module (from_modules); weights are packed once, there."""

    def __init__(self, stem, stages, inner, outer, dtype=torch.float32):
        self.stem, self.stages, self.inner, self.outer, self.dtype = stem, stages, inner, outer, _dtype(dtype)
        if len(inner) != len(stages) or len(outer) != len(stages):
            raise ValueError(f'the FPN holds {len(inner)} lateral and {len(outer)} output blocks for {len(stages)} stages')
        width = stem.c_out
        for blocks, lat, lay in zip(stages, inner, outer):
            for blk in blocks:
                if blk.conv1.c_in != width:
                    raise ValueError(f'{blk.conv1.name}: expects {blk.conv1.c_in} channels, the layer before it gives {width}')
                width = blk.conv3.c_out
            if lat.c_in != width or lay.c_in != lat.c_out or lay.c_out != outer[0].c_out or lat.c_out != inner[0].c_out:
                raise ValueError(f'{lat.name}: the FPN\'s widths do not match the stage ({width}) or one another')
        self._arena = {}
        self.trainable, self.train_from_stage, self.train_dtype = False, None, None
        self.keep_rows, self.timer, self.last_rows, self.last_kept_bytes = False, None, None, 0

    # ---- construction ----
    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float32, device=None, prefix='backbone.', trainable=False, train_from_stage=2, train_dtype=None):
        """torchvision 0.4.2's keys under `prefix`: body.conv1 / bn1, body.layer{s}.{i}.conv{1,2,3} / bn{1,2,3} / downsample.{0,1}, fpn.inner_blocks.{l},
        fpn.layer_blocks.{l}.  Block counts and widths are the keys' and the shapes'; num_batches_tracked and every other key are ignored; a
        missing key is a KeyError naming it.
        trainable (float32 parameters): the conv weights of body.layer{train_from_stage}.. and the FPN's weights and biases are
        torch.nn.Parameters on the device under torchvision's names; the stem, the stages below and every FrozenBatchNorm stay constants.
        train_from_stage = stages + 1 trains the FPN alone; 0 (the stem and the pool) is refused: their backward is not built.
        dtype stays the type of the parameters: float32, the master weights.  train_dtype names the type of the rows and
        of the packed weights: None or torch.float32: section 29's path; torch.bfloat16: bfloat16 rows kept for the backward, bfloat16 gradient
        rows, the frozen stages packed once in bfloat16, float32 .grad; torch.float16 is refused (no loss scaler)"""
        from .detector_trunk_backward import check_train_dtype
        dtype = _dtype(dtype)
        row_dtype = check_train_dtype(trainable, train_dtype)
        kw = dict(dtype=dtype, device=device)
        if trainable:
            if dtype != torch.float32:
                raise ValueError(f'a trainable trunk is float32 only (dtype is the type of the parameters, the master weights; 16-bit rows are '
                                 f'train_dtype=torch.bfloat16), got dtype={dtype}')
            if isinstance(train_from_stage, bool) or not isinstance(train_from_stage, int):
                raise ValueError(f'train_from_stage must be an int, got {train_from_stage!r}')
            if train_from_stage < 1:
                raise ValueError(f'train_from_stage={train_from_stage}: the backward of the 7x7 stem and of the 3x3 max pool is not built; the first '
                                 'trainable stage is body.layer1 (train_from_stage=1)')
            if device is None:
                first = next((t for t in sd.values() if torch.is_tensor(t) and t.is_cuda), None)
                device = first.device if first is not None else None
            if device is None or torch.device(device).type != 'cuda':
                raise ValueError(f'a trainable trunk lives on the ROCm device: give device=, got {device}')
            kw.update(device=device, dtype=row_dtype)
            from .detector_trunk_backward import TrainableTrunkLayer
            counter = [0]

        def get(key):
            if prefix + key not in sd:
                raise KeyError(prefix + key)
            t = sd[prefix + key]
            if key.endswith('.weight') and t.dim() == 4 and (t.shape[0] % 8 or (t.shape[1] % 8 and t.shape[1] != 3)):
                raise ValueError(f'{prefix}{key[:-7]}: {int(t.shape[1])} -> {int(t.shape[0])} channels: every channel count but the image\'s 3 '
                                 'must be a multiple of 8 (the rows between the layers are not padded silently)')
            return t

        def bn(name):
            return tuple(get(f'{name}.{part}') for part in _BN)

        def conv_bn(conv, norm, stride=1, relu=True, train=False):
            if train:
                return TrainableTrunkLayer(prefix + conv, get(conv + '.weight'), bn=bn(norm), stride=stride, relu=relu, device=device, counter=counter, dtype=row_dtype)
            return TrunkLayer(prefix + conv, get(conv + '.weight'), bn=bn(norm), stride=stride, relu=relu, **kw)

        def fpn_layer(key):
            if trainable:
                return TrainableTrunkLayer(prefix + key, get(key + '.weight'), bias=get(key + '.bias'), device=device, counter=counter, dtype=row_dtype)
            return TrunkLayer(prefix + key, get(key + '.weight'), bias=get(key + '.bias'), **kw)
        found = {}
        for k in sd:
            m = re.match(re.escape(prefix) + r'body\.layer(\d+)\.(\d+)\.', k)
            if m:
                found.setdefault(int(m.group(1)), set()).add(int(m.group(2)))
        if not found:
            raise KeyError(prefix + 'body.layer1.0.conv1.weight')
        if trainable and train_from_stage > max(found) + 1:
            raise ValueError(f'train_from_stage={train_from_stage} exceeds {max(found) + 1} (the {max(found)} stages + 1: the FPN alone)')
        stem = conv_bn('body.conv1', 'body.bn1', stride=2)
        stages = []
        for s in range(1, max(found) + 1):
            blocks = []
            t = bool(trainable) and s >= train_from_stage
            for i in range(max(found.get(s, {0})) + 1):
                p = f'body.layer{s}.{i}'
                stride = 2 if (s > 1 and i == 0) else 1               # ResNet v1.5: the stride sits on the 3x3 and on downsample.0
                down = None
                if any(k.startswith(f'{prefix}{p}.downsample.') for k in sd):
                    down = conv_bn(f'{p}.downsample.0', f'{p}.downsample.1', stride=stride, relu=False, train=t)
                blocks.append(Bottleneck(conv_bn(f'{p}.conv1', f'{p}.bn1', train=t), conv_bn(f'{p}.conv2', f'{p}.bn2', stride=stride, train=t),
                                         conv_bn(f'{p}.conv3', f'{p}.bn3', train=t), down))       # conv3's ReLU follows the shortcut's add
            stages.append(blocks)
        inner = [fpn_layer(f'fpn.inner_blocks.{l}') for l in range(len(stages))]
        outer = [fpn_layer(f'fpn.layer_blocks.{l}') for l in range(len(stages))]
        for lay in outer:
            if lay.ksize != 3:
                raise ValueError(f'{lay.name}: an FPN output block is a 3x3 convolution, got {lay.ksize}x{lay.ksize}')
        trunk = cls(stem, stages, inner, outer, row_dtype if trainable else dtype)      # self.dtype: the rows' type
        if trainable:
            trunk.train_dtype = row_dtype
            trunk._init_trainable(sd, prefix, train_from_stage, counter)
        return trunk

    @classmethod
    def from_modules(cls, backbone, dtype=torch.float32, device=None, trainable=False, train_from_stage=2, train_dtype=None):
        """the same from a module with torchvision's attribute names (body, fpn): its state_dict under no prefix (trainable: copies, never
        the module's own tensors)"""
        sd = backbone.state_dict()
        if device is None:
            first = next(iter(sd.values())).device
            device = first if first.type != 'cpu' else None
        return cls.from_state_dict(sd, dtype, device, prefix='', trainable=trainable, train_from_stage=train_from_stage, train_dtype=train_dtype)

    # ---- the trainable trunk ----
    def _init_trainable(self, sd, prefix, train_from_stage, counter):
        self.trainable, self.train_from_stage, self._counter, self._prefix = True, int(train_from_stage), counter, prefix
        self._named = []
        for layer in self.layers():
            if hasattr(layer, 'weight'):
                self._named += [(f'{layer.name}.{part}', p) for part, p in zip(('weight', 'bias'), layer.parameters())]
        own = re.compile(re.escape(prefix) + r'(body|fpn)\.')
        trained = {k for k, _ in self._named}
        # every key of the trunk, in the state dict's order: parameters by reference, the frozen weights and the BatchNorm buffers as CPU copies
        self._keys = [k for k in sd if own.match(k)]
        self._frozen = {k: sd[k].detach().to('cpu').clone() for k in self._keys if k not in trained}

    def _need_trainable(self, what):
        if not self.trainable:
            raise RuntimeError(f'{what}: this DetectorTrunk is inference only; build it with trainable=True')

    @property
    def pack_count(self):
        """device weight packs launched so far: one per layer whose parameters moved since its last pack"""
        self._need_trainable('pack_count')
        return self._counter[0]

    def named_parameters(self):
        self._need_trainable('named_parameters')
        return list(self._named)

    def parameters(self):
        self._need_trainable('parameters')
        return [t for _, t in self._named]

    def zero_grad(self):
        for t in self.parameters():
            t.grad = None

    def state_dict(self):
        """ALL the trunk's keys under the prefix it was built with, the frozen layers and the BatchNorm buffers included: detached copies"""
        self._need_trainable('state_dict')
        live = dict(self._named)
        return {k: (live[k].detach().clone() if k in live else self._frozen[k].clone()) for k in self._keys}

    def load_state_dict(self, sd, strict=True):
        """copies the trainable keys into the parameters in place (their _version moves, the next forward packs again).  The frozen keys are
        constants of this trunk: a value that differs from the one it was built with is refused (build a new trunk from that state dict)"""
        self._need_trainable('load_state_dict')
        for k, t in self._named:
            if k not in sd:
                if strict:
                    raise KeyError(k)
                continue
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f'{k} must be {tuple(t.shape)}, got {tuple(sd[k].shape)}')
        for k, t in self._frozen.items():
            if k in sd and not k.endswith('num_batches_tracked') and not torch.equal(sd[k].detach().to('cpu', t.dtype), t):
                raise ValueError(f'{k} is frozen in this trunk and differs from the value it was built with: build a new trunk with from_state_dict')
        with torch.no_grad():
            for k, t in self._named:
                if k in sd:
                    t.copy_(sd[k])

    def layers(self):
        """every packed layer, in a fixed order (tests compare their bytes)"""
        return [self.stem] + [l for blocks in self.stages for blk in blocks for l in blk.layers()] + self.inner + self.outer

    def block(self, stage, i):
        """the i-th bottleneck of body.layer{stage} (stage from 1): block(x (B,C,H,W) float32) -> (B,C',Ho,Wo) float32"""
        return self.stages[stage - 1][i]

    # ---- the arena: one flat buffer per slot, grown on demand, reused from call to call ----
    def _buf(self, name, rows, channels):
        n = rows * channels
        flat = self._arena.get(name)
        if flat is None or flat.numel() < n or flat.device != self._dev:
            flat = self._arena[name] = torch.empty(max(n, 1), dtype=self.dtype, device=self._dev)
        return flat[:n].view(rows, channels)

    def arena_bytes(self):
        return sum(t.numel() * t.element_size() for t in self._arena.values())

    def _ready(self, dev):
        self._dev = dev
        for layer in self.layers():
            layer.ready(dev)

    # ---- the forward pass ----
    def stem_rows(self, images):
        """images -> the pooled stem's rows, H, W: stem pack, the stem GEMM (scale, shift, ReLU), the 3x3 stride-2 pool"""
        B, _, H, W = (int(v) for v in images.shape)
        Hs, Ws = _out2(H, W)
        cols = self._buf('stem_cols', B * Hs * Ws, STEM_ROW)
        if B:
            _lib.check(_lib.lib().cosy_trunk_stem_pack(_lib.ptr(images), _lib.ptr(cols), B, H, W, _DTYPES[self.dtype], _lib.stream()))
        s = _trunk_gemm(self.stem, cols, B, Hs, Ws, self._buf('stem', B * Hs * Ws, self.stem.c_out))
        H, W = _out2(Hs, Ws)
        return max_pool_rows(s, B, Hs, Ws, self._buf('pooled', B * H * W, self.stem.c_out)), H, W

    def stage_rows(self, x, B, H, W):
        """the pooled stem's rows -> [(rows, H, W)] of every stage's output, in the arena"""
        outs, flip = [], 0
        for si, blocks in enumerate(self.stages):
            for bi, blk in enumerate(blocks):
                name = f'stage{si}' if bi == len(blocks) - 1 else f'x{flip}'      # a stage's output stays until the FPN has read it
                x, H, W = blk.rows(x, B, H, W, self._buf, name)
                flip ^= 1
            outs.append((x, H, W))
        return outs

    def fpn_rows(self, feats, B):
        """stage outputs [(rows, H, W)] -> the output maps as views of one flat float32 buffer, then the 'pool' level"""
        L, C = len(feats), self.outer[0].c_out
        starts = [0]
        for _, H, W in feats:
            starts.append(starts[-1] + B * H * W)
        if starts[-1] > MAX_ROWS:
            raise ValueError(f'{starts[-1]} rows (cells of all levels) exceed the limit of 2^30 per launch')
        inner = self._buf('inner', starts[-1], self.inner[0].c_out)
        for l in range(L - 1, -1, -1):                                  # top-down: the coarser lateral is the residual of the finer one
            x, H, W = feats[l]
            res, res_hw = (None, None) if l == L - 1 else (inner[starts[l + 1]:starts[l + 2]], feats[l + 1][1:])
            _trunk_gemm(self.inner[l], x, B, H, W, inner[starts[l]:starts[l + 1]], residual=res, res_hw=res_hw)
        dev = inner.device
        flat = torch.empty(C * starts[-1], dtype=torch.float32, device=dev)
        maps = [(B, H, W) for _, H, W in feats]
        for l, (n, H, W) in enumerate(maps):                            # every level has weights of its own: one launch per level
            _gemm(self.outer[l], inner[starts[l]:starts[l + 1]], [(n, H, W)], _lib.HEAD_STORE_NCHW, flat[C * starts[l]:C * starts[l + 1]])
        out = [flat[C * starts[l]:C * starts[l + 1]].view(B, C, H, W) for l, (_, H, W) in enumerate(maps)]
        out.append(out[-1][..., ::2, ::2].contiguous())                  # LastLevelMaxPool: max_pool2d(x, 1, 2, 0), a strided subsample
        return out

    def fpn(self, feats):
        """the FPN alone: the stage outputs as (B,C_l,H_l,W_l) float32 maps (rounded to the storage type on the way in) -> the five maps"""
        if not isinstance(feats, (list, tuple)) or len(feats) != len(self.stages):
            raise ValueError(f'the FPN takes the list of the {len(self.stages)} stage outputs, got {len(feats) if isinstance(feats, (list, tuple)) else type(feats).__name__}')
        feats = [_input(f, f'feats[{l}]', self.inner[l].c_in) for l, f in enumerate(feats)]
        self._ready(feats[0].device)
        B = int(feats[0].shape[0])
        return self.fpn_rows([(_to_rows(f, self.dtype), int(f.shape[2]), int(f.shape[3])) for f in feats], B)

    def __call__(self, images):
        if self.trainable and torch.is_grad_enabled() and torch.is_tensor(images) and images.requires_grad:
            raise RuntimeError('images requires grad: the backward of the 7x7 stem and of the 3x3 max pool is not built; detach the input')
        images = _input(images, 'images', 3)
        self._ready(images.device)
        with torch.cuda.device(images.device):
            if self.trainable and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                from .detector_trunk_backward import TrunkFn
                out = list(TrunkFn.apply(self, images, *self.parameters()))
                return out + [out[-1][..., ::2, ::2].contiguous()]      # LastLevelMaxPool: a torch slice of the node's last output
            B = int(images.shape[0])
            x, H, W = self.stem_rows(images)
            return self.fpn_rows(self.stage_rows(x, B, H, W), B)


ANCHOR_SIZES = ((32,), (64,), (128,), (256,), (512,))      # the reference's DetectorMaskRCNN
ASPECT_RATIOS = (0.5, 1.0, 2.0)                              # at every level


class Detector:
    """The reference's cosypose.integrated.detector.Detector: uint8 frames in, the `detections` collection out, every layer in between on this
    package's kernels.  The Mask R-CNN options are torchvision 0.4.2's defaults with the reference's anchors."""

    def __init__(self, trunk, heads, label_to_category_id, input_resize=(480, 640)):
        self.trunk, self.heads = trunk, heads
        self.label_to_category_id = dict(label_to_category_id)
        self.category_id_to_label = {v: k for k, v in self.label_to_category_id.items()}
        self.min_size, self.max_size = int(min(input_resize)), int(max(input_resize))

    @classmethod
    def from_state_dict(cls, sd, label_to_category_id, input_resize=(480, 640), dtype=torch.float32, device='cuda', trainable=False, train_from_stage=2,
                        train_dtype=None, heads_train_dtype=None):
        """a reference detector checkpoint's state_dict as it is (backbone.*, rpn.head.*, roi_heads.*).  trainable: the trainable trunk
         and the trainable heads (section 28), float32 parameters.  train_dtype=torch.bfloat16: the trunk runs section
        30's bfloat16 rows; its maps are float32 NCHW, so the float32 trainable heads follow it unchanged.  heads_train_dtype=torch.bfloat16:
        the heads run section 32's bfloat16 rows (None: float32 rows); both together are the fully 16-bit training step"""
        from .detector_heads import DetectorHeads
        from .detector_trunk_backward import check_train_dtype
        check_train_dtype(trainable, train_dtype)
        check_train_dtype(trainable, heads_train_dtype, 'heads')
        if trainable and dtype != torch.float32:
            raise ValueError(f'a trainable detector is float32 only (dtype is the type of the parameters; bfloat16 rows in the trunk are '
                             f'train_dtype=torch.bfloat16), got dtype={dtype}')
        trunk = DetectorTrunk.from_state_dict(sd, dtype, device, trainable=trainable, train_from_stage=train_from_stage, train_dtype=train_dtype)
        heads = DetectorHeads.from_state_dict(sd, dtype, device, trainable=trainable, train_dtype=heads_train_dtype)
        return cls(trunk, heads, label_to_category_id, input_resize)

    # ---- training (trainable=True): the reference's train_detector.py loop on this library's kernels ----
    @property
    def trainable(self):
        return bool(getattr(self.trunk, 'trainable', False) and getattr(self.heads, 'trainable', False))

    def _need_trainable(self, what):
        if not self.trainable:
            raise RuntimeError(f'{what}: this Detector is inference only; build it with trainable=True')

    def losses(self, frames, targets, keys=None, generator=None):
        """uint8 frames and their targets (boxes, labels, masks at the frames' sizes) -> the reference's loss_dict, with autograd history
        through the heads, both RoIAligns and the trunk; the detector's sizes and the RPN settings of get_detections"""
        from .detector_input import detector_losses_from_frames
        self._need_trainable('losses')
        return detector_losses_from_frames(frames, targets, self.trunk, self.heads.rpn_head, self.heads.box_head, self.heads.mask_head,
                                           min_size=self.min_size, max_size=self.max_size, keys=keys, generator=generator, sizes=ANCHOR_SIZES,
                                           aspect_ratios=ASPECT_RATIOS)

    def named_parameters(self):
        self._need_trainable('named_parameters')
        return self.trunk.named_parameters() + self.heads.named_parameters()

    def parameters(self):
        return [t for _, t in self.named_parameters()]

    def zero_grad(self):
        for t in self.parameters():
            t.grad = None

    def optimizer(self, **kw):
        """detector_optim.FlatSGD over this detector's parameters (lr=, momentum=, weight_decay=): its step keeps the packings of every trainable
        layer of the trunk and the heads current with one launch"""
        from .detector_heads import PackedOnDevice
        from .detector_optim import FlatSGD
        self._need_trainable('optimizer')
        return FlatSGD(self, layers=[l for l in self.trunk.layers() + self.heads.layers() if isinstance(l, PackedOnDevice)], **kw)

    def state_dict(self):
        self._need_trainable('state_dict')
        return {**self.trunk.state_dict(), **self.heads.state_dict()}

    def load_state_dict(self, sd, strict=True):
        self._need_trainable('load_state_dict')
        self.trunk.load_state_dict(sd, strict)
        self.heads.load_state_dict(sd, strict)

    def train(self, mode=True):
        """nothing here has a mode (every BatchNorm is frozen, there is no dropout): returns self"""
        return self

    def eval(self):
        return self

    def get_detections(self, images, detection_th=None, output_masks=False, mask_th=0.8, one_instance_per_class=False):
        """images: uint8 frames (B,H,W,3) or (B,3,H,W), or a list of them; float frames are refused (detector_input)"""
        from .detector_input import detections_from_frames
        with torch.no_grad():
            return detections_from_frames(images, self.trunk, self.heads.rpn_head, self.heads.box_head, self.heads.mask_head, self.category_id_to_label,
                                          min_size=self.min_size, max_size=self.max_size, detection_th=detection_th, output_masks=output_masks,
                                          mask_th=mask_th, one_instance_per_class=one_instance_per_class, sizes=ANCHOR_SIZES,
                                          aspect_ratios=ASPECT_RATIOS)

    def __call__(self, *args, **kwargs):
        return self.get_detections(*args, **kwargs)

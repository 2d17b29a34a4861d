"""The cases that tests/test_detector_trunk_host.py (CPU), tests/test_detector_trunk.py and tests/test_detector_e2e.py (GPU) share: seeded layers of
the detector's trunk at the smallest shapes at which cosy_trunk_conv takes each of its paths, and one narrow ResNet-50-shaped state dict under
torchvision's names.  The twin's references are computed once per process and handed out unchanged."""
import functools

import numpy as np

import dettrunk_ref as ref

F32 = np.float32
DTYPES = ('float32', 'float16', 'bfloat16')
SALT = 1                                 # chosen so that frames_ref.fma32's DoubleRounding guard fires on no case (test_detector_trunk_host.py)

# (name, ksize, stride, C_in, C_out, store, (B, H, W), scale?, residual (rH, rW) or None, relu)
MAPS = [(5, 7), (4, 6), (1, 2), (2, 1)]
STRIDED = [(f's2-k{k}-c{ci}-{st}{co}-{H}x{W}', k, 2, ci, co, st, (2, H, W), True, None, True)
           for k in (1, 3) for ci in (40, 8) for co, st in ((24, 'rows'), (15, 'nchw')) for H, W in MAPS]
RESIDUAL = [('s1-identity-residual', 3, 1, 40, 24, 'rows', (2, 5, 7), True, (5, 7), True),
            ('up-5x7-from-3x4', 1, 1, 40, 24, 'rows', (2, 5, 7), False, (3, 4), False),
            ('up-6x10-from-3x5', 1, 1, 8, 24, 'nchw', (2, 6, 10), False, (3, 5), False)]
# 1 x 50 x 82 at stride 2 -> 25 x 41 = 1025 output rows = 4 row tiles of 256 + 1: the large row tile and its last partial tile, by OUTPUT rows
BIG = [('s2-1025-rows', 3, 2, 8, 24, 'rows', (1, 50, 82), True, None, True), ('s2-1025-rows-88', 1, 2, 40, 88, 'nchw', (1, 50, 82), True, None, False)]
CASES = STRIDED + RESIDUAL + BIG
STEMS = [(2, 3, 9, 11), (1, 3, 8, 8), (1, 3, 1, 1)]
POOLS = [(2, 8, 5, 7), (1, 16, 4, 6), (1, 8, 1, 1)]


def case_id(case):
    return case[0]


def _rng(name):
    return np.random.RandomState(SALT + sum(ord(c) * (i + 1) for i, c in enumerate(name)))


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> twin layer dict, input x (B,C,H,W) float32, residual (B,O,rH,rW) float32 or None"""
    name, k, stride, ci, co, store, (B, H, W), scaled, res, relu = case
    rng = _rng(name)
    w = (rng.normal(0, 1, (co, ci, k, k)) / np.sqrt(ci * k * k)).astype(F32)
    layer = dict(weight=w, stride=stride, scale=rng.uniform(0.5, 1.5, co).astype(F32) * rng.choice([-1, 1], co).astype(F32) if scaled else None,
                 bias=rng.normal(0, 0.5, co).astype(F32), relu=bool(relu))
    x = rng.normal(0, 1, (B, ci, H, W)).astype(F32)
    r = None if res is None else rng.normal(0, 1, (B, co) + tuple(res)).astype(F32)
    return layer, x, r


@functools.lru_cache(maxsize=None)
def want64(case, dtype):
    """-> value, bound (K + 3) u A of the twin's float64 evaluation fed the operands rounded to dtype"""
    layer, x, r = case_data(case)
    v, A, K = ref.layer64(layer, x, r, dtype)
    return v, (K + 3) * ref.U[dtype] * A


@functools.lru_cache(maxsize=None)
def want32(case):
    return ref.layer32(*case_data(case))


@functools.lru_cache(maxsize=None)
def stem_data(shape):
    """-> twin stem layer (over stem_columns), the (O,3,7,7) weight, scale, shift, images"""
    rng = _rng('stem' + 'x'.join(map(str, shape)))
    w = (rng.normal(0, 1, (8, 3, 7, 7)) / np.sqrt(147)).astype(F32)
    scale, shift = rng.uniform(0.5, 1.5, 8).astype(F32), rng.normal(0, 0.5, 8).astype(F32)
    return ref.stem_layer(w, scale, shift), w, scale, shift, rng.normal(0, 1, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def pool_data(shape):
    """all values negative (a zero padding would win every border window), one NaN"""
    rng = _rng('pool' + 'x'.join(map(str, shape)))
    x = (np.round(-rng.uniform(0.5, 4, shape) * 8) / 8).astype(F32)             # multiples of 1/8 below 4: exact in every storage type
    x[0, shape[1] - 1, shape[2] // 2, shape[3] // 2] = np.nan
    return x


# ---- the narrow ResNet-50-shaped trunk: stem 8; planes 8/16/24/32, expansion 4; blocks 3/4/6/3; FPN width 16 -------------------------------
STEM_C, PLANES, BLOCKS, EXPANSION, FPN_C = 8, (8, 16, 24, 32), (3, 4, 6, 3), 4, 16
INPUTS = [(2, 3, 64, 64), (2, 3, 45, 77)]


@functools.lru_cache(maxsize=None)
def trunk_weights(seed=7, prefix='backbone.'):
    """{name: float32 array} under torchvision 0.4.2's names, with num_batches_tracked entries and a head key that the loader must ignore"""
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, o, c, k):
        sd[f'{prefix}{name}.weight'] = (rng.normal(0, 1, (o, c, k, k)) * np.sqrt(2.0 / (c * k * k))).astype(F32)

    def bn(name, o, gain=1.0):
        sd[f'{prefix}{name}.weight'] = (rng.uniform(0.5, 1.5, o) * gain).astype(F32)
        sd[f'{prefix}{name}.bias'] = rng.normal(0, 0.2, o).astype(F32)
        sd[f'{prefix}{name}.running_mean'] = rng.normal(0, 0.2, o).astype(F32)
        sd[f'{prefix}{name}.running_var'] = rng.uniform(0.5, 2.0, o).astype(F32)
        sd[f'{prefix}{name}.num_batches_tracked'] = np.array(0, np.int64)
    conv('body.conv1', STEM_C, 3, 7), bn('body.bn1', STEM_C)
    width = STEM_C
    for s, (planes, n) in enumerate(zip(PLANES, BLOCKS), 1):
        for i in range(n):
            p = f'body.layer{s}.{i}'
            conv(p + '.conv1', planes, width, 1), bn(p + '.bn1', planes)
            conv(p + '.conv2', planes, planes, 3), bn(p + '.bn2', planes)
            conv(p + '.conv3', planes * EXPANSION, planes, 1), bn(p + '.bn3', planes * EXPANSION, 0.5)
            if i == 0:
                conv(p + '.downsample.0', planes * EXPANSION, width, 1), bn(p + '.downsample.1', planes * EXPANSION, 0.5)
            width = planes * EXPANSION
    for l, planes in enumerate(PLANES):
        for kind, c, k in (('inner_blocks', planes * EXPANSION, 1), ('layer_blocks', FPN_C, 3)):
            conv(f'fpn.{kind}.{l}', FPN_C, c, k)
            sd[f'{prefix}fpn.{kind}.{l}.bias'] = rng.normal(0, 0.1, FPN_C).astype(F32)
    sd['rpn.head.conv.bias'] = np.zeros(FPN_C, F32)
    return sd


@functools.lru_cache(maxsize=None)
def trunk_net():
    return ref.net_from_sd(trunk_weights())


@functools.lru_cache(maxsize=None)
def trunk_images(shape):
    return _rng('images' + 'x'.join(map(str, shape))).normal(0, 1, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def trunk_bits(shape):
    """the five float32 maps as chained fmaf chains, and the stage outputs"""
    keep = {}
    return ref.trunk32(trunk_net(), trunk_images(shape), keep), keep['feats']


@functools.lru_cache(maxsize=None)
def trunk_emulated(shape, dtype, store=True):
    """the storage-emulating chain: the five (value, bound), every block's input value and the stage outputs"""
    keep = {}
    return ref.trunk(trunk_net(), trunk_images(shape), dtype, store, keep), keep


def torch_trunk(sd=None, prefix='backbone.'):
    """the same network as plain torch.nn modules under torchvision's attribute names (body, fpn), float64-capable, eval, no grad:
    -> module whose forward returns the five maps"""
    import torch
    import torch.nn.functional as F
    from torch import nn
    sd = trunk_weights() if sd is None else sd
    has = lambda k: prefix + k in sd
    shape = lambda k: sd[prefix + k].shape

    class FrozenBN(nn.Module):
        def __init__(self, n):
            super().__init__()
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                self.register_buffer(k, torch.ones(n))

        def forward(self, x):
            scale = self.weight.float() * self.running_var.float().rsqrt()             # in float32 whatever the module's type (section 27)
            shift = self.bias.float() - self.running_mean.float() * scale
            return x * scale.to(x.dtype).reshape(1, -1, 1, 1) + shift.to(x.dtype).reshape(1, -1, 1, 1)

    def conv(key, stride=1, bias=False):
        o, c, k, _ = shape(key + '.weight')
        return nn.Conv2d(c, o, k, stride, k // 2, bias=bias)

    class Block(nn.Module):
        def __init__(self, p, stride):
            super().__init__()
            self.conv1, self.bn1 = conv(p + '.conv1'), FrozenBN(shape(p + '.conv1.weight')[0])
            self.conv2, self.bn2 = conv(p + '.conv2', stride), FrozenBN(shape(p + '.conv2.weight')[0])
            self.conv3, self.bn3 = conv(p + '.conv3'), FrozenBN(shape(p + '.conv3.weight')[0])
            self.downsample = None
            if has(p + '.downsample.0.weight'):
                self.downsample = nn.Sequential(conv(p + '.downsample.0', stride), FrozenBN(shape(p + '.downsample.0.weight')[0]))

        def forward(self, x):
            out = torch.relu(self.bn1(self.conv1(x)))
            out = torch.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return torch.relu(out + (x if self.downsample is None else self.downsample(x)))

    class Body(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, shape('body.conv1.weight')[0], 7, 2, 3, bias=False)
            self.bn1 = FrozenBN(shape('body.conv1.weight')[0])
            s = 1
            while has(f'body.layer{s}.0.conv1.weight'):
                blocks, i = [], 0
                while has(f'body.layer{s}.{i}.conv1.weight'):
                    blocks.append(Block(f'body.layer{s}.{i}', 2 if (s > 1 and i == 0) else 1))
                    i += 1
                setattr(self, f'layer{s}', nn.Sequential(*blocks))
                s += 1
            self.n = s - 1

        def forward(self, x):
            x = F.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
            out = []
            for s in range(1, self.n + 1):
                x = getattr(self, f'layer{s}')(x)
                out.append(x)
            return out

    class FPN(nn.Module):
        def __init__(self, n):
            super().__init__()
            self.inner_blocks = nn.ModuleList([conv(f'fpn.inner_blocks.{l}', bias=True) for l in range(n)])
            self.layer_blocks = nn.ModuleList([conv(f'fpn.layer_blocks.{l}', bias=True) for l in range(n)])

        def forward(self, feats):
            last = self.inner_blocks[-1](feats[-1])
            out = [self.layer_blocks[-1](last)]
            for l in range(len(feats) - 2, -1, -1):
                lateral = self.inner_blocks[l](feats[l])
                last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode='nearest')
                out.insert(0, self.layer_blocks[l](last))
            return out + [F.max_pool2d(out[-1], 1, 2, 0)]

    class Backbone(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = Body()
            self.fpn = FPN(self.body.n)

        def forward(self, x):
            return self.fpn(self.body(x))

    m = Backbone()
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(np.asarray(sd[prefix + k])).reshape(own[k].shape) for k in own})
    return m.eval().requires_grad_(False)


# ---- end to end: the trunk's weights joined with head weights over the FPN's 16 channels ---------------------------------------------------
E2E_FRAMES = [(37, 53), (45, 40)]
E2E_LABELS = {'obj_000001': 1, 'obj_000002': 2}


@functools.lru_cache(maxsize=None)
def detector_weights(seed=11):
    """trunk_weights() with head weights in the style of dethead_case.chain_weights() over FPN_C channels (the RPN's SIZE deltas are zero, so
    the proposals are bit-equal on the device and in the twin)"""
    import dethead_case as hc
    rng = np.random.RandomState(seed)
    C, A, K = FPN_C, 3, hc.K
    sd = dict(trunk_weights())
    del sd['rpn.head.conv.bias']

    def put(name, shape, scale, bias=0.1):
        sd[name + '.weight'] = (rng.normal(0, 1, shape) * scale).astype(F32)
        sd[name + '.bias'] = (rng.normal(0, 1, shape[1] if 'conv5_mask' in name else shape[0]) * bias).astype(F32)
    put('rpn.head.conv', (C, C, 3, 3), 0.2)
    put('rpn.head.cls_logits', (A, C, 1, 1), 0.3)
    put('rpn.head.bbox_pred', (4 * A, C, 1, 1), 0.3)
    sd['rpn.head.bbox_pred.weight'].reshape(A, 4, C)[:, 2:] = 0
    sd['rpn.head.bbox_pred.bias'].reshape(A, 4)[:, 2:] = 0
    put('roi_heads.box_head.fc6', (16, C * 49), 0.3 / 7)
    put('roi_heads.box_head.fc7', (16, 16), 0.3)
    put('roi_heads.box_predictor.cls_score', (K, 16), 0.4)
    put('roi_heads.box_predictor.bbox_pred', (4 * K, 16), 0.06)
    for i in range(1, 5):
        put(f'roi_heads.mask_head.mask_fcn{i}', (C, C, 3, 3), 0.2)
    put('roi_heads.mask_predictor.conv5_mask', (C, C, 2, 2), 0.5)
    put('roi_heads.mask_predictor.mask_fcn_logits', (K, C, 1, 1), 1.0)
    return sd

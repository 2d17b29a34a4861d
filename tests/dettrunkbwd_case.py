"""The cases that tests/test_detector_trunk_backward_host.py (CPU) and tests/test_detector_trunk_backward.py (GPU) share: seeded layers at the
smallest shapes at which cosy_trunk_dgrad and cosy_trunk_wgrad take each of their paths, and the narrow trunk of dettrunk_case.py with seeded
gradients on its five maps.  The twin's references are computed once per process and handed out unchanged."""
import functools

import numpy as np

import dettrunk_case as tc
import dettrunk_ref as tref
import dettrunkbwd_ref as ref

F32 = np.float32
MAPS = tc.MAPS                                   # dX maps 5x7, 4x6, 1x2, 2x1: an even H has a last row whose only tap would read past the output map
SLAB = 256

# data gradient: (name, ksize, stride, C_in, C_out, (B, H, W) of dX, adds [(rule, (h, w))], mask)
DGRAD = [(f'd-s2-k3-c{ci}-24-{H}x{W}', 3, 2, ci, 24, (2, H, W), (), False) for ci in (40, 8) for H, W in MAPS]
DGRAD += [(f'd-s1-k3-c{ci}-24-{H}x{W}-same-mask', 3, 1, ci, 24, (2, H, W), ((ref.SAME, (H, W)),), True) for ci in (40, 8) for H, W in MAPS]
DGRAD += [('d-nearest-3x4-from-5x7', 3, 1, 16, 16, (2, 3, 4), ((ref.NEAREST_T, (5, 7)),), False),
          ('d-nearest-3x5-from-6x10', 3, 1, 16, 16, (2, 3, 5), ((ref.NEAREST_T, (6, 10)),), False),
          ('d-two-adds-even-same-mask-5x7', 1, 1, 40, 24, (2, 5, 7), ((ref.EVEN, (3, 4)), (ref.SAME, (5, 7))), True),
          ('d-two-adds-same-nearest-4x6', 3, 1, 8, 24, (2, 4, 6), ((ref.SAME, (4, 6)), (ref.NEAREST_T, (7, 12))), True),
          # 1 x 50 x 82 at stride 2: every parity class holds 25 x 41 = 1025 rows: the large row tile and its last partial tile
          ('d-s2-1025-rows', 3, 2, 8, 24, (1, 50, 82), (), True)]
# a 1x1 at stride 2 (downsample.0): its data gradient runs on the OUTPUT grid and enters a dX of (H, W) through EVEN
EVEN_CASES = [('even-5x7', (2, 5, 7)), ('even-4x6', (2, 4, 6))]

# weight gradient: (name, ksize, stride, C_in, C_out, (B, H, W) of x, scale: True, False (an FPN layer: a bias gradient) or 'negative')
WGRAD = [(f'w-s2-k{k}-T{Wp}', k, 2, 8, 24, (1, 2, 2 * Wp - 1), True) for k in (3, 1) for Wp in (SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3)]
WGRAD += [(f'w-s2-k{k}-c40-{H}x{W}', k, 2, 40, 24, (2, H, W), True) for k in (3, 1) for H, W in MAPS]
WGRAD += [('w-negative-scale', 3, 2, 8, 24, (2, 5, 7), 'negative'), ('w-fpn-k3', 3, 1, 16, 16, (2, 5, 7), False), ('w-fpn-k1', 1, 1, 40, 16, (2, 4, 6), False),
          ('w-s1-k1-c88', 1, 1, 88, 24, (2, 5, 7), True)]


def case_id(case):
    return case[0]


def _rng(name):
    return np.random.RandomState(tc.SALT + sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _layer(rng, k, stride, ci, co, scaled=True):
    w = (rng.normal(0, 1, (co, ci, k, k)) / np.sqrt(ci * k * k)).astype(F32)
    scale = None
    if scaled:
        scale = rng.uniform(0.5, 1.5, co).astype(F32) * rng.choice([-1, 1], co).astype(F32)
        if scaled == 'negative':
            scale = -np.abs(scale)
    return dict(weight=w, stride=stride, scale=scale, bias=rng.normal(0, 0.5, co).astype(F32), relu=True)


def _mask_rows(rng, shape):
    """stored rows of the layer below: positive, negative, exact zeros and one -0.0"""
    y = rng.normal(0, 1, shape).astype(F32)
    y[rng.uniform(0, 1, shape) < 0.2] = 0
    y.reshape(-1)[0] = -0.0
    return y


@functools.lru_cache(maxsize=None)
def dgrad_data(case):
    """-> layer, g (B,O,Ho,Wo), adds [(rule, map)], y or None"""
    name, k, stride, ci, co, (B, H, W), adds, mask = case
    rng = _rng(name)
    layer = _layer(rng, k, stride, ci, co)
    g = rng.normal(0, 1, (B, co, tref.out_size(H, stride), tref.out_size(W, stride))).astype(F32)
    ops = [(rule, rng.normal(0, 1, (B, ci) + tuple(hw)).astype(F32)) for rule, hw in adds]
    return layer, g, ops, _mask_rows(rng, (B, ci, H, W)) if mask else None


@functools.lru_cache(maxsize=None)
def dgrad_want(case):
    layer, g, ops, y = dgrad_data(case)
    H, W = case[5][1:]
    return ref.dx32(layer, g, H, W, ops, y)


@functools.lru_cache(maxsize=None)
def even_data(case):
    """downsample.0 (16 -> 8 channels seen from the gradient: O = 16 outputs, C = 8 inputs) and the conv1 whose launch takes its rows through EVEN.
    Cell (1, 1) of image 0 -- odd -- is made to hold -0.0 in channel 0 of conv1's accumulator: every product there is a negative underflow.
    -> down layer, conv1 layer, g3 (B,16,Ho,Wo), g1 (B,16,H,W)"""
    name, (B, H, W) = case
    rng = _rng(name)
    down, conv1 = _layer(rng, 1, 2, 8, 16), _layer(rng, 1, 1, 8, 16)
    conv1['scale'] = np.abs(conv1['scale'])
    conv1['weight'][:, 0] = F32(1e-20)
    g3 = rng.normal(0, 1, (B, 16, tref.out_size(H, 2), tref.out_size(W, 2))).astype(F32)
    g1 = rng.normal(0, 1, (B, 16, H, W)).astype(F32)
    if H > 1 and W > 1:
        g1[0, :, 1, 1] = F32(-1e-30)
    return down, conv1, g3, g1


@functools.lru_cache(maxsize=None)
def even_want(case):
    down, conv1, g3, g1 = even_data(case)
    B, H, W = case[1]
    d = ref.dx32(ref.on_output_grid(down), g3, *g3.shape[2:])
    return d, ref.dx32(conv1, g1, H, W, [(ref.EVEN, d)])


@functools.lru_cache(maxsize=None)
def wgrad_data(case):
    """-> layer, x (B,C,H,W), g (B,O,Ho,Wo)"""
    name, k, stride, ci, co, (B, H, W), scaled = case
    rng = _rng(name)
    layer = _layer(rng, k, stride, ci, co, scaled)
    x = rng.normal(0, 1, (B, ci, H, W)).astype(F32)
    return layer, x, rng.normal(0, 1, (B, co, tref.out_size(H, stride), tref.out_size(W, stride))).astype(F32)


@functools.lru_cache(maxsize=None)
def wgrad_want(case):
    return ref.wgrad64(*wgrad_data(case))


# ---- the narrow trunk ------------------------------------------------------------------------------------------------------------------------------
N_STAGES = len(tc.BLOCKS)
TRAIN_FROM = (2, 1, N_STAGES + 1)


@functools.lru_cache(maxsize=None)
def trunk_grads(shape, nan=False):
    """seeded gradients at the five maps (the forward's shapes); nan: one NaN planted in the gradient of map '2'"""
    rng = _rng('grads' + 'x'.join(map(str, shape)))
    out = [rng.normal(0, 1, m.shape).astype(F32) for m in trunk_forward(shape)['out']]
    if nan:
        out[2][1, 3, out[2].shape[2] // 2, out[2].shape[3] // 2] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def trunk_forward(shape):
    return ref.forward_keep(tc.trunk_net(), tc.trunk_images(shape))


@functools.lru_cache(maxsize=None)
def trunk_want(shape, train_from_stage=1, nan=False):
    """the twin's backward of the float32 chain.  The chain from the top is the same whatever the first trainable stage is: a later
    train_from_stage names a subset of these results (`trained`)"""
    return ref.trunk_backward(tc.trunk_net(), tc.trunk_images(shape), trunk_grads(shape, nan), train_from_stage, keep=trunk_forward(shape))


def trained(name, train_from_stage):
    """does a parameter or a row buffer of this name exist with this first trainable stage"""
    if name.startswith('fpn.G_inner') or name.startswith('fpn.inner_blocks') or name.startswith('fpn.layer_blocks'):
        return True
    if name.startswith('fpn.lateral_dx.'):
        return int(name.rsplit('.', 1)[1]) + 1 >= train_from_stage
    s = int(name.split('.')[1][len('layer'):])                                 # body.layer{s}.{i}.*
    if name.endswith('.down_dx'):
        return s > train_from_stage
    return s >= train_from_stage


def torch_sd():
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in tc.trunk_weights().items()}

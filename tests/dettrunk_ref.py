"""numpy restatement of DESIGN.md section 27: the layers of the detector's trunk (ResNet bottlenecks with FrozenBatchNorm, the FPN) as the device
computes them.  Independent of the package: nothing here imports cosypose_amd.  It extends tests/dethead_ref.py, whose summation order,
rounding helpers and bound it reuses.

A layer is a dict: weight (O,C,k,k) with k = 1 or 3 (pad k // 2), stride 1 or 2, scale (O) float32 or None, bias (O) float32 (the shift), relu.
A residual is a (B,O,rH,rW) map; output cell (y, x) takes its cell (min(floor(y sy), rH - 1), min(floor(x sx), rW - 1)), sy = float32(rH) / float32(Ho),
the product in float32 (torch's legacy mode='nearest'; rH == Ho: the identity).

Epilogue per output: v = fmaf(acc, scale, bias) (scale None: acc + bias), v = v + r (one rounded add), ReLU as x < 0 ? 0 : x, the store's type.
  * layer64: float64 -> value, A = |scale| sum |w x| + |bias| + |r|, K: the tests' bound is (K + 3) u A (K roundings of the chain, one of the
    fused scale / shift, one of the residual add);
  * layer32: the float32 fmaf chain in the kernel's order (dethead_ref.layer32's) with that epilogue;
  * step: one layer of a storage-emulating chain with its running bound; bottleneck / fpn / trunk chain the steps, bottleneck32 / fpn32 / trunk32
    the fmaf chains.
"""
import numpy as np

import dethead_ref as ref
from frames_ref import fma32

F32 = np.float32
U = ref.U
STEM_ROW = 152


def out_size(n, stride):
    return (n - 1) // stride + 1


def nearest_index(n_in, n_out):
    """source index of every output index of one axis, torch's legacy nearest: min(floor(dst * float32(in) / float32(out)), in - 1)"""
    scale = F32(n_in) / F32(n_out)
    prod = np.arange(n_out, dtype=F32) * scale
    assert prod.dtype == F32
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def upsample(r, Ho, Wo):
    """(B,C,rH,rW) -> (B,C,Ho,Wo) by the nearest rule"""
    return r[:, :, nearest_index(r.shape[2], Ho)][:, :, :, nearest_index(r.shape[3], Wo)]


def columns(x, k, stride):
    """(B,C,H,W) -> (B,Ho,Wo,k*k,C): the taps of every output cell, (ky, kx) ascending, zeros outside the map"""
    B, C, H, W = x.shape
    p, Ho, Wo = k // 2, out_size(H, stride), out_size(W, stride)
    xp = np.zeros((B, C, H + 2 * p, W + 2 * p), x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    taps = [xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(k) for kx in range(k)]
    return np.stack(taps, 1).transpose(0, 3, 4, 1, 2)


def stem_columns(images):
    """(B,3,H,W) -> (B,152,Ho,Wo): element (ky 7 + kx) 3 + c of output cell (y, x) is images[b, c, 2y - 3 + ky, 2x - 3 + kx], +0.0 outside the
    image, elements 147..151 +0.0.  The stem is then a 1x1 layer of 152 channels (stem_layer)."""
    B, C, H, W = images.shape
    Ho, Wo = out_size(H, 2), out_size(W, 2)
    xp = np.zeros((B, C, H + 6, W + 6), images.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = images
    out = np.zeros((B, STEM_ROW, Ho, Wo), images.dtype)
    for ky in range(7):
        for kx in range(7):
            out[:, (ky * 7 + kx) * 3:(ky * 7 + kx) * 3 + 3] = xp[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
    return out


def stem_layer(weight, scale, bias, relu=True):
    """the 7x7 stride-2 stem (O,3,7,7) as the one-tap layer over stem_columns"""
    O = weight.shape[0]
    w = np.zeros((O, STEM_ROW, 1, 1), weight.dtype)
    w[:, :147, 0, 0] = weight.transpose(0, 2, 3, 1).reshape(O, 147)
    return dict(weight=w, stride=1, scale=scale, bias=bias, relu=relu)


def maxpool(x):
    """max_pool2d(3, 2, 1): padding -inf, v > m || isnan(v) takes v, the taps (ky, kx) ascending"""
    B, C, H, W = x.shape
    Ho, Wo = out_size(H, 2), out_size(W, 2)
    xp = np.full((B, C, H + 2, W + 2), -np.inf, x.dtype)
    xp[:, :, 1:1 + H, 1:1 + W] = x
    m = np.full((B, C, Ho, Wo), -np.inf, x.dtype)
    with np.errstate(invalid='ignore'):
        for ky in range(3):
            for kx in range(3):
                v = xp[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
                m = np.where((v > m) | np.isnan(v), v, m)
    return m


def relu(y):
    return ref.relu(y)


def _gemm_view(layer, x):
    w = np.asarray(layer['weight'])
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    cols = columns(x, k, layer.get('stride', 1))
    B, Ho, Wo = cols.shape[:3]
    return cols.reshape(B * Ho * Wo, k * k, C), w.transpose(0, 2, 3, 1).reshape(O, k * k, C), (B, Ho, Wo, O)


def _back(y, shape):
    B, Ho, Wo, O = shape
    return y.reshape(B, Ho, Wo, O).transpose(0, 3, 1, 2)


def layer64(layer, x, residual=None, dtype=None):
    """float64 evaluation -> value, A, K.  dtype: round x, the weight and the residual to that storage type first (scale and bias stay float32)"""
    x = np.asarray(x, np.float64)
    rows, w, shape = _gemm_view(layer, x)
    w = w.astype(np.float64)
    r = None if residual is None else np.asarray(residual, np.float64)
    if dtype is not None:
        rows, w = ref.round_to(rows, dtype), ref.round_to(w, dtype)
        r = None if r is None else ref.round_to(r, dtype)
    M, T, C = rows.shape
    r2, w2 = rows.reshape(M, T * C), w.reshape(-1, T * C)
    y, S = _back(r2 @ w2.T, shape), _back(np.abs(r2) @ np.abs(w2).T, shape)
    b = np.asarray(layer['bias'], np.float64)[None, :, None, None]
    if layer.get('scale') is not None:
        s = np.asarray(layer['scale'], np.float64)[None, :, None, None]
        y, S = y * s, S * np.abs(s)
    y, A = y + b, S + np.abs(b)
    if r is not None:
        up = upsample(r, shape[1], shape[2])
        y, A = y + up, A + np.abs(up)
    if layer.get('relu'):
        y = relu(y)
    return y, A, T * C


def layer32(layer, x, residual=None):
    """the float32 fmaf chain in the kernel's order, then the trunk's epilogue -> float32 array"""
    rows, w, shape = _gemm_view(layer, np.asarray(x, F32))
    rows, w = rows.astype(F32), w.astype(F32)
    M, T, C = rows.shape
    acc = np.zeros((M, w.shape[0]), F32)
    with np.errstate(invalid='ignore'):
        for c0 in range(0, C, ref.KB32):
            for t in range(T):
                for c in (c0 + 4 * g + e for e in range(4) for g in range(4)):
                    if c < C:
                        acc = fma32(rows[:, t, c][:, None], w[:, t, c][None, :], acc)
        b = np.asarray(layer['bias'], F32)[None, :]
        if layer.get('scale') is not None:
            y = fma32(acc, np.asarray(layer['scale'], F32)[None, :], b)
        else:
            y = (acc + b).astype(F32)
        y = _back(y, shape)
        if residual is not None:
            y = (y + upsample(np.asarray(residual, F32), shape[1], shape[2])).astype(F32)
    if layer.get('relu'):
        y = relu(y)
    return np.ascontiguousarray(y)


def step(layer, value, err, dtype, residual=None, stored=True):
    """one layer of a storage-emulating chain.  value: what the storage type holds (float64), err: a bound on |device - value| (or None);
    residual: (value, err) likewise.  -> value, err of the output, rounded to the storage type where `stored` (16-bit types only)"""
    u = U[dtype]
    w = ref.round_to(layer['weight'], dtype)
    lay = dict(layer, weight=w)
    rv, re = (None, None) if residual is None else residual
    y, A, K = layer64(lay, value, rv)
    carried = np.zeros_like(A)
    if err is not None:
        absl = dict(weight=np.abs(w), stride=layer.get('stride', 1), scale=None if layer.get('scale') is None else np.abs(layer['scale']),
                    bias=np.zeros(w.shape[0], F32), relu=False)
        carried = layer64(absl, err)[0]
    if re is not None:
        carried = carried + upsample(re, y.shape[2], y.shape[3])
    err = carried + (K + 3) * u * (A + carried)
    if stored and dtype != 'float32':
        err = err + ref.storage_ulp(np.abs(y) + err, dtype)
        y = ref.round_to(y, dtype)
    return y, err


def bottleneck(blk, value, err, dtype, store=True):
    """conv1, conv2, the optional downsample, conv3 with the shortcut and the ReLU in its epilogue -> value, err.  store=False: no
    intermediate is rounded to the storage type (the measure of the whole-trunk limit)"""
    a = step(blk['conv1'], value, err, dtype, stored=store)
    b = step(blk['conv2'], *a, dtype, stored=store)
    short = (value, err if err is not None else np.zeros_like(value))
    if blk.get('down') is not None:
        short = step(blk['down'], value, err, dtype, stored=store)
    return step(blk['conv3'], *b, dtype, residual=short, stored=store)


def bottleneck32(blk, x):
    a = layer32(blk['conv1'], x)
    b = layer32(blk['conv2'], a)
    short = x if blk.get('down') is None else layer32(blk['down'], x)
    return layer32(blk['conv3'], b, short)


def fpn(net, feats, dtype, store=True):
    """feats: [(value, err)] of the stage outputs -> [(value, err)] of the five maps; the laterals are stored as rows, the outputs are float32"""
    L = len(feats)
    inner = [None] * L
    for l in range(L - 1, -1, -1):
        inner[l] = step(net['inner'][l], *feats[l], dtype, residual=None if l == L - 1 else inner[l + 1], stored=store)
    out = [step(net['outer'][l], *inner[l], dtype, stored=False) for l in range(L)]
    out.append((out[-1][0][..., ::2, ::2], out[-1][1][..., ::2, ::2]))
    return out


def fpn32(net, feats):
    L = len(feats)
    inner = [None] * L
    for l in range(L - 1, -1, -1):
        inner[l] = layer32(net['inner'][l], feats[l], None if l == L - 1 else inner[l + 1])
    out = [layer32(net['outer'][l], inner[l]) for l in range(L)]
    return out + [np.ascontiguousarray(out[-1][..., ::2, ::2])]


def trunk(net, images, dtype, store=True, keep=None):
    """the storage-emulating chain of the whole trunk -> [(value, err)] of the five maps.  The images and every weight are rounded to `dtype`;
    store=False rounds no intermediate.  keep: a dict that receives every block's input value under (stage, i) and the stage outputs under 'feats'"""
    x = ref.round_to(stem_columns(np.asarray(images, np.float64)), dtype)
    v, e = step(net['stem'], x, None, dtype, stored=store)
    v, e = maxpool(v), _pool_err(e)
    feats = []
    for s, blocks in enumerate(net['stages']):
        for i, blk in enumerate(blocks):
            if keep is not None:
                keep[(s + 1, i)] = v
            v, e = bottleneck(blk, v, e, dtype, store)
        feats.append((v, e))
    if keep is not None:
        keep['feats'] = [f[0] for f in feats]
    return fpn(net, feats, dtype, store)


def _pool_err(e):
    """a bound on the pooled value's error: the largest bound in the window (max is 1-Lipschitz in the sup norm)"""
    B, C, H, W = e.shape
    Ho, Wo = out_size(H, 2), out_size(W, 2)
    ep = np.zeros((B, C, H + 2, W + 2), e.dtype)
    ep[:, :, 1:1 + H, 1:1 + W] = e
    return np.max([ep[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2] for ky in range(3) for kx in range(3)], 0)


def trunk32(net, images, keep=None):
    """the float32 trunk as chained fmaf chains: what the device computes in float32, bit for bit -> the five maps"""
    v = maxpool(layer32(net['stem'], stem_columns(np.asarray(images, F32))))
    feats = []
    for s, blocks in enumerate(net['stages']):
        for i, blk in enumerate(blocks):
            v = bottleneck32(blk, v)
        feats.append(v)
    if keep is not None:
        keep['feats'] = feats
    return fpn32(net, feats)


# ---- the network from a state_dict-like {name: array} under torchvision 0.4.2's names -----------------------------------------------------
def frozen_bn(sd, name):
    """FrozenBatchNorm2d (no eps) -> scale, shift in float32: scale = weight * rsqrt(running_var), shift = bias - running_mean * scale, every
    operation rounded on its own"""
    w, b, m, v = (np.asarray(sd[f'{name}.{k}'], F32) for k in ('weight', 'bias', 'running_mean', 'running_var'))
    scale = (w * (F32(1) / np.sqrt(v))).astype(F32)
    return scale, (b - (m * scale).astype(F32)).astype(F32)


def net_from_sd(sd, prefix='backbone.'):
    def conv_bn(conv, bn, stride=1, relu=True):
        scale, shift = frozen_bn(sd, prefix + bn)
        return dict(weight=np.asarray(sd[f'{prefix}{conv}.weight'], F32), stride=stride, scale=scale, bias=shift, relu=relu)
    stem = conv_bn('body.conv1', 'body.bn1')
    net = dict(stem=stem_layer(stem['weight'], stem['scale'], stem['bias']), stages=[], inner=[], outer=[])
    s = 1
    while f'{prefix}body.layer{s}.0.conv1.weight' in sd:
        blocks, i = [], 0
        while f'{prefix}body.layer{s}.{i}.conv1.weight' in sd:
            p, stride = f'body.layer{s}.{i}', 2 if (s > 1 and i == 0) else 1
            down = conv_bn(f'{p}.downsample.0', f'{p}.downsample.1', stride, False) if f'{prefix}{p}.downsample.0.weight' in sd else None
            blocks.append(dict(conv1=conv_bn(f'{p}.conv1', f'{p}.bn1'), conv2=conv_bn(f'{p}.conv2', f'{p}.bn2', stride),
                               conv3=conv_bn(f'{p}.conv3', f'{p}.bn3'), down=down))
            i += 1
        net['stages'].append(blocks)
        s += 1
    for l in range(len(net['stages'])):
        for kind in ('inner', 'outer'):
            key = f'{prefix}fpn.{"inner" if kind == "inner" else "layer"}_blocks.{l}'
            net[kind].append(dict(weight=np.asarray(sd[key + '.weight'], F32), stride=1, scale=None, bias=np.asarray(sd[key + '.bias'], F32), relu=False))
    return net

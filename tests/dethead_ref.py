"""numpy restatement of DESIGN.md section 26: the layers of the detector's heads (3x3 / 1x1 conv, linear, ConvTranspose2d(k=2, s=2)) as
the device computes them.  Independent of the package: nothing here imports cosypose_amd.

Three evaluations of one layer out = act(W x + bias):
  * layer64: float64, and with every value S = sum |w x| + |bias| and the reduction length K -- the measure of the tests' bound
    |got - want| <= (K + 2) u S (u = 2^-24 for float32: an fmaf chain of K terms plus one bias add; 2^-23 for the 16-bit types against this
    evaluation fed the ROUNDED operands: their products are exact in float32 and K additions of any order, truncating adders included, stay
    inside it);
  * layer32: the float32 fmaf chain in the kernel's order -- accumulator +0.0, the channels in blocks of 16 ascending, inside a block the taps
    (ky, kx) ascending, inside a tap the block's channels in the order 4 g + e, e = 0..3 outside, g = 0..3 inside (a tap outside the map feeds 0, which leaves the accumulator as it is), one
    rounded bias add, ReLU as x < 0 ? 0 : x -- through frames_ref.fma32, whose DoubleRounding guard refuses a sum it cannot promise;
  * chain: layers one after the other with the storage type emulated (operands and stored intermediates rounded to nearest even) and a running
    error bound e_out = sum |w| e_in + (K + 2) u (S + sum |w| e_in), plus one storage ulp of |y| + e where a 16-bit intermediate is stored.
    ReLU does not enlarge a bound.

A layer is a dict: kind 'conv' (weight (O,C,k,k), k = 3 pad 1 or k = 1), 'linear' (weight (O,K)) or 'deconv' (weight (C,O,2,2)), bias, relu.
"""
import numpy as np

from frames_ref import fma32

F32 = np.float32
KB32 = 16                                      # channels per k-block of the float32 kernel
U = {'float32': 2.0 ** -24, 'float16': 2.0 ** -23, 'bfloat16': 2.0 ** -23}


def round_to(x, dtype):
    """float array -> float64 array of the values the storage type holds (round to nearest even; float16 overflows to inf like torch)"""
    x = np.asarray(x, np.float64)
    if dtype == 'float32':
        return x.astype(F32).astype(np.float64)
    if dtype == 'float16':
        with np.errstate(over='ignore'):
            return x.astype(F32).astype(np.float16).astype(np.float64)
    if dtype == 'bfloat16':
        bits = np.ascontiguousarray(x.astype(F32)).view(np.uint32).astype(np.uint64)
        rounded = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16 << 16).astype(np.uint32)
        out = rounded.view(F32).astype(np.float64)
        return np.where(np.isnan(x), np.nan, out)
    raise ValueError(dtype)


def storage_ulp(y, dtype):
    """one unit in the last place of the storage type at |y| (float64 array)"""
    bits, emin = {'float16': (10, -14), 'bfloat16': (7, -126)}[dtype]
    e = np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - bits)


def columns(x, k):
    """(B,C,H,W) -> (B,H,W,k*k,C): the taps of every cell, (ky, kx) ascending, zeros outside the map"""
    B, C, H, W = x.shape
    p = k // 2
    xp = np.zeros((B, C, H + 2 * p, W + 2 * p), x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    return np.stack([xp[:, :, ky:ky + H, kx:kx + W] for ky in range(k) for kx in range(k)], 1).transpose(0, 3, 4, 1, 2)


def as_gemm(layer, x):
    """-> rows (M, T, C) of x, weight (N, T, C), bias (N), and the function that puts (M, N) back into the layer's output shape"""
    w, kind = np.asarray(layer['weight']), layer['kind']
    b = np.asarray(layer['bias']) if layer.get('bias') is not None else None
    if kind == 'linear':
        M = x.shape[0]
        return x.reshape(M, 1, w.shape[1]), w.reshape(w.shape[0], 1, -1), b, lambda y: y
    B, C, H, W = x.shape
    if kind == 'conv':
        O, k = w.shape[0], w.shape[2]
        rows = columns(x, k).reshape(B * H * W, k * k, C)
        return rows, w.transpose(0, 2, 3, 1).reshape(O, k * k, C), b, lambda y: y.reshape(B, H, W, O).transpose(0, 3, 1, 2)
    if kind == 'deconv':
        O = w.shape[1]
        rows = x.transpose(0, 2, 3, 1).reshape(B * H * W, 1, C)
        w2 = w.reshape(C, O * 4).T.reshape(O * 4, 1, C)                      # column (o, dy, dx)
        b4 = None if b is None else np.repeat(b, 4)
        return rows, w2, b4, lambda y: y.reshape(B, H, W, O, 2, 2).transpose(0, 3, 1, 4, 2, 5).reshape(B, O, 2 * H, 2 * W)
    raise ValueError(kind)


def relu(y):
    return np.where(y < 0, np.zeros_like(y), y)                               # a NaN stays NaN, as torch's


def layer64(layer, x, dtype=None):
    """float64 evaluation -> value, S, K.  dtype: round x and the weight to that storage type first (the bias stays float32)"""
    x = np.asarray(x, np.float64)
    rows, w, b, back = as_gemm(layer, x)
    w = w.astype(np.float64)
    if dtype is not None:
        rows, w = round_to(rows, dtype), round_to(w, dtype)
    M, T, C = rows.shape
    r2, w2 = rows.reshape(M, T * C), w.reshape(-1, T * C)
    y, S = r2 @ w2.T, np.abs(r2) @ np.abs(w2).T
    if b is not None:
        y, S = y + b.astype(np.float64), S + np.abs(b.astype(np.float64))
    if layer.get('relu'):
        y = relu(y)
    return back(y), back(S), T * C


def layer32(layer, x):
    """the float32 fmaf chain in the kernel's order -> float32 array"""
    rows, w, b, back = as_gemm(layer, np.asarray(x, F32))
    rows, w = rows.astype(F32), w.astype(F32)
    M, T, C = rows.shape
    acc = np.zeros((M, w.shape[0]), F32)
    with np.errstate(invalid='ignore'):
        for c0 in range(0, C, KB32):
            for t in range(T):
                for c in (c0 + 4 * g + e for e in range(4) for g in range(4)):   # MFMA e of the block sums the channels 4 g + e, g ascending
                    if c < C:
                        acc = fma32(rows[:, t, c][:, None], w[:, t, c][None, :], acc)
        y = (acc + (np.zeros(w.shape[0], F32) if b is None else b.astype(F32))[None, :]).astype(F32)
    if layer.get('relu'):
        y = relu(y)
    return back(y)


def chain(layers, x, dtype, stores=None, err0=None):
    """layers one after the other as the device runs them -> value (float64), bound on |device - value|.  The input and every weight are rounded
    to `dtype`; every output but the last is stored in `dtype` (stores: one bool per layer, default all but the last).  err0: the inputs of the device may
    differ from x by up to that much (float32 only: a rounded input would add its own ulp)"""
    u = U[dtype]
    value, err = round_to(x, dtype), err0                                     # err0: a bound on |device input - x|, same shape as x
    stores = [True] * (len(layers) - 1) + [False] if stores is None else stores
    for layer, stored in zip(layers, stores):
        w = round_to(layer['weight'], dtype)                                  # `value` already holds what the storage type holds
        y, S, K = layer64(dict(layer, weight=w), value)
        rows_w = dict(layer, bias=None, relu=False, weight=np.abs(w))
        carried = np.zeros_like(S) if err is None else layer64(rows_w, err)[0]
        err = carried + (K + 2) * u * (S + carried)
        value = y
        if stored and dtype != 'float32':
            err = err + storage_ulp(np.abs(value) + err, dtype)
            value = round_to(value, dtype)
    return value, err


def chain32(layers, x):
    """the float32 fmaf chains one after the other: what the device computes in float32, bit for bit"""
    for layer in layers:
        x = layer32(layer, x)
    return x


# ---- the three heads as lists of layers, from a state_dict-like {name: array} -----------------------------------------------------------
def rpn_layers(sd):
    conv = dict(kind='conv', weight=sd['rpn.head.conv.weight'], bias=sd['rpn.head.conv.bias'], relu=True)
    pred = dict(kind='conv', weight=np.concatenate([sd['rpn.head.cls_logits.weight'], sd['rpn.head.bbox_pred.weight']]),
                bias=np.concatenate([sd['rpn.head.cls_logits.bias'], sd['rpn.head.bbox_pred.bias']]), relu=False)
    return [conv, pred]


def rpn_head(sd, feats, dtype):
    """-> per level (objectness, deltas) values and bounds: [(obj, e_obj, dl, e_dl)]"""
    out = []
    A = sd['rpn.head.cls_logits.weight'].shape[0]
    for f in feats:
        v, e = chain(rpn_layers(sd), f, dtype)
        out.append((v[:, :A], e[:, :A], v[:, A:], e[:, A:]))
    return out


def box_layers(sd):
    p = 'roi_heads.box_'
    return [dict(kind='linear', weight=sd[p + 'head.fc6.weight'], bias=sd[p + 'head.fc6.bias'], relu=True),
              dict(kind='linear', weight=sd[p + 'head.fc7.weight'], bias=sd[p + 'head.fc7.bias'], relu=True),
              dict(kind='linear', weight=np.concatenate([sd[p + 'predictor.cls_score.weight'], sd[p + 'predictor.bbox_pred.weight']]),
                   bias=np.concatenate([sd[p + 'predictor.cls_score.bias'], sd[p + 'predictor.bbox_pred.bias']]), relu=False)]


def box_head(sd, roi, dtype):
    K = sd['roi_heads.box_predictor.cls_score.weight'].shape[0]
    v, e = chain(box_layers(sd), np.asarray(roi).reshape(len(roi), -1), dtype)
    return v[:, :K], e[:, :K], v[:, K:], e[:, K:]


def mask_layers(sd):
    layers = [dict(kind='conv', weight=sd[f'roi_heads.mask_head.mask_fcn{i}.weight'], bias=sd[f'roi_heads.mask_head.mask_fcn{i}.bias'], relu=True)
              for i in range(1, 5)]
    layers.append(dict(kind='deconv', weight=sd['roi_heads.mask_predictor.conv5_mask.weight'], bias=sd['roi_heads.mask_predictor.conv5_mask.bias'], relu=True))
    layers.append(dict(kind='conv', weight=sd['roi_heads.mask_predictor.mask_fcn_logits.weight'], bias=sd['roi_heads.mask_predictor.mask_fcn_logits.bias'],
                       relu=False))
    return layers


def mask_head(sd, roi, dtype):
    return chain(mask_layers(sd), roi, dtype)

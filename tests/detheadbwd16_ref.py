"""numpy restatement of DESIGN.md section 32: the backward of the detector's heads on bfloat16 rows under float32 master weights.  Independent
of the package: nothing here imports cosypose_amd.  tests/dettrunkbwd16_ref.py supplies the rounding and the 16-bit fragment order,
tests/detheadbwd_ref.py the heads' index rules (tap order, the deconvolution's cells, torchvision's layouts) and the float64 sums; both are
imported, not edited.  A layer is dethead_ref's dict (siblings: one concatenated weight).

  * pack_fwd16 / pack_bwd16 / bias_pad: the bytes cosy_head_weight_pack16 writes; grad_rows: those of cosy_head_grad_pack16.
  * dgrad64: ONE data-gradient launch in float64 on the bf16-exact operands given to it (ws = the packed weight's values, g, y): t64,
    S = sum |ws g|, K = taps x the o summed, blocked = where the mask stores +0.0.  dgrad_bound: b = (K + 2) 2^-23 S, the bound of the float32
    accumulator (what an NCHW store writes), and b + 2^-8 (|t64| + b), the bound of a row store's one rounding to bfloat16.
  * wgrad64 / wgrad_bound: ONE weight gradient in float64 on bf16-exact x and g: (T + 2) 2^-23 S_W and (T + 1) 2^-23 S_b, T the cells summed
    (the rows of x; the deconvolution's bias: the rows of g).
  * dgrad_f32 / wgrad_f32: float32-accumulate emulations (numpy's order, not the hardware's) that show the bounds are not vacuous.
"""
import numpy as np

import dethead_ref as ref
import detheadbwd_ref as bref
from dettrunkbwd16_ref import U16, UB, bf16, bf16_bits, from_bits, is_bf16, pack16, pack16_at  # noqa: F401  (the tests reach them here)

F32 = np.float32


def pad8(n):
    return -(-n // 8) * 8


def layer16(layer):
    """the layer as the 16-bit launches see it: the weight rounded once to bfloat16 (the values of both packings), the bias float32"""
    return dict(layer, weight=bf16(np.asarray(layer['weight'], F32)))


def fwd_operand(layer):
    """(N, taps, C) bf16-exact: the forward GEMM's weight as dethead_ref.as_gemm states it (deconv: the 4 C_o rows (o, dy, dx), one tap)"""
    w, kind = bf16(np.asarray(layer['weight'], F32)), layer['kind']
    if kind == 'linear':
        return w.reshape(w.shape[0], 1, w.shape[1])
    if kind == 'conv':
        return w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1])
    return w.reshape(w.shape[0], -1).T.reshape(-1, 1, w.shape[0])


def bwd_operand(layer):
    """(C, taps, O) bf16-exact as detheadbwd_ref.dgrad_operands states it: rows c, reduction o, taps reversed (conv) or (dy, dx) ascending (deconv)"""
    w, kind = bf16(np.asarray(layer['weight'], F32)), layer['kind']
    if kind == 'linear':
        return w.T.reshape(w.shape[1], 1, w.shape[0])
    if kind == 'conv':
        return w[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(w.shape[1], -1, w.shape[0])
    return w.transpose(0, 2, 3, 1).reshape(w.shape[0], 4, w.shape[1])


def pack_fwd16(layer):
    return pack16(np.ascontiguousarray(fwd_operand(layer)))


def pack_bwd16(layer):
    return pack16(np.ascontiguousarray(bwd_operand(layer)))


def bias_pad(layer):
    b = np.asarray(layer['bias'], F32)
    if layer['kind'] == 'deconv':
        b = np.repeat(b, 4)
    out = np.zeros(-(-len(b) // 64) * 64, F32)
    out[:len(b)] = b
    return out


def grad_rows(g0, g1=None):
    """NCHW (B, n0, ...) and (B, n1, ...) float32 (None: zeros of no columns) -> uint16 rows (B HW, pad8(n0 + n1)): g0's columns, g1's, then +0.0"""
    parts = [np.asarray(g, F32).reshape(g.shape[0], g.shape[1], -1) for g in (g0, g1) if g is not None]
    g = np.concatenate(parts, 1)
    B, n, HW = g.shape
    rows = np.zeros((B * HW, pad8(n)), F32)
    rows[:, :n] = g.transpose(0, 2, 1).reshape(B * HW, n)
    return bf16_bits(rows)


# ---- one data-gradient launch ----------------------------------------------------------------------------------------------------------
def dgrad64(layer, g, y=None):
    """layer: its weight as packed (layer16); g the gradient in the layer's output shape, y the stored input-shaped rows or None: the values
    the launch reads (bf16-exact on the device) -> dict(t64, S, K, blocked) in the shape of the layer's input"""
    w = np.asarray(layer['weight'])
    g = np.asarray(g, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        t = bref.dx64(layer, g)
        S = bref.dx64(dict(layer, weight=np.abs(w)), np.abs(g))
    taps = 4 if layer['kind'] == 'deconv' else 1 if layer['kind'] == 'linear' else w.shape[2] * w.shape[3]
    O = w.shape[1] if layer['kind'] == 'deconv' else w.shape[0]
    blocked = np.zeros(t.shape, bool) if y is None else np.asarray(y) <= 0
    return dict(t64=t, S=S, K=taps * O, blocked=blocked)


def dgrad_bound(d):
    """-> b (the float32 accumulator against t64: the NCHW store), b16 (a row store's bfloat16 against t64)"""
    b = (d['K'] + 2) * U16 * d['S']
    return b, b + UB * (np.abs(d['t64']) + b)


def dgrad_f32(layer, g, y=None, rows=True):
    """a float32-accumulate emulation of the launch: products exact, numpy's float32 sums, the mask, one rounding (rows) or none (NCHW)"""
    rws, wt, back = bref.dgrad_operands(layer, np.asarray(g, F32))
    acc = np.zeros((rws.shape[0], wt.shape[0]), F32)
    for t in range(rws.shape[1]):
        for o in range(rws.shape[2]):
            acc = (acc + (rws[:, t, o][:, None].astype(np.float64) * wt[:, t, o][None, :]).astype(F32)).astype(F32)
    v = back(acc)
    if y is not None:
        v = bref.relu_mask(y, v)
    return bf16(v) if rows else v


# ---- one weight gradient ---------------------------------------------------------------------------------------------------------------
def wgrad64(layer, x, g):
    """x in the layer's input shape, g in its output shape: the values the launch reads (bf16-exact on the device) -> detheadbwd_ref.wgrad64's
    dict (float64, torchvision's layout)"""
    return bref.wgrad64(layer, x, g)


def wgrad_bound(d):
    return (d['T_W'] + 2) * U16 * d['S_W'], (d['T_b'] + 1) * U16 * d['S_b']


def wgrad_f32(layer, x, g):
    """float32-accumulate emulation: the cells in ascending order, one rounded add per cell -> dW, db in torchvision's layout"""
    rows = ref.as_gemm(layer, np.asarray(x, np.float64))[0]
    g2 = bref.gemm_columns(layer, np.asarray(g, np.float64))
    M, T, C = rows.shape
    r2 = rows.reshape(M, T * C)
    acc, accb = np.zeros((g2.shape[1], T * C), F32), np.zeros(g2.shape[1], F32)
    for m in range(M):
        acc = (acc + np.outer(g2[m], r2[m]).astype(F32)).astype(F32)
        accb = (accb + g2[m].astype(F32)).astype(F32)
    w = np.asarray(layer['weight'])
    if layer['kind'] == 'conv':
        return acc.reshape(w.shape[0], w.shape[2], w.shape[3], C).transpose(0, 3, 1, 2), accb
    if layer['kind'] == 'linear':
        return acc, accb
    O = w.shape[1]
    return acc.reshape(O, 2, 2, C).transpose(3, 0, 1, 2), accb.reshape(O, 4).sum(1, dtype=F32)

"""numpy restatement of DESIGN.md section 30: the backward of the detector's trunk on bfloat16 rows under float32 master weights.  Independent
of the package: nothing here imports cosypose_amd.  tests/dettrunkbwd_ref.py (section 29) supplies `spread`, the NEAREST_T cells, the add rules
and the float64 sums; it is imported, not edited.

  * bf16: float32 -> the nearest bfloat16 (ties to even, a NaN stays a NaN), returned as float32 values; bf16_bits: the 16 bits.
  * pack16: the 16-bit fragment order of cosy_head_conv (k-blocks of 32, eight elements per lane); pack_fwd16 / pack_bwd16: the bytes
    cosy_trunk_weight_pack16 writes; ws16 = bf16(fl32(w scale[o])): one float32 product, then one rounding.
  * dgrad64: ONE data-gradient launch in float64 on the bf16-exact operands given to it: t64 (accumulate, then the adds in order, before the
    mask), S = sum |ws g| + sum |add terms|, K = the live taps times the o summed, n = the add terms taken, blocked = where the mask stores +0.0.
    dgrad_bound: the bound on the float32 value handed to the conversion and the bound on the stored bfloat16.
  * wgrad64 / wgrad_bound16: ONE weight gradient in float64 on bf16-exact operands, and section 29's bound with the 16-bit unit 2^-23.
  * dgrad_f32 / wgrad_f32: a float32-accumulate emulation (numpy's order, not the hardware's) that shows the bounds are not vacuous.
"""
import numpy as np

import dettrunk_ref as tref
import dettrunkbwd_ref as ref

F32 = np.float32
U16 = 2.0 ** -23          # one float32 addition that may truncate (section 26): the unit of every float32 accumulation of 16-bit products
UB = 2.0 ** -8            # one rounding to bfloat16's 8 significand bits, relative
SAME, EVEN, NEAREST_T = ref.SAME, ref.EVEN, ref.NEAREST_T


def bf16_bits(a):
    """float32 -> uint16: round to nearest, ties to even; a NaN keeps its sign and becomes quiet"""
    a = np.ascontiguousarray(a, F32)
    u = a.view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = np.isnan(a)
    rounded = np.where(nan, (u >> 16) | 0x40, rounded)
    return rounded.astype(np.uint16).reshape(a.shape)


def from_bits(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(F32).reshape(np.shape(b))


def bf16(a):
    return from_bits(bf16_bits(a))


def is_bf16(a):
    a = np.ascontiguousarray(a, F32)
    return bool(((a.view(np.uint32) & 0xFFFF) == 0).all())


def ws16(weight, scale=None):
    w = np.asarray(weight, F32)
    if scale is not None:
        w = (w * np.asarray(scale, F32)[:, None, None, None]).astype(F32)
    return bf16(w)


def pack16(w):
    """(N, taps, K) bf16-exact float32 -> uint16 [N_pad / 16][tap][k-block][lane = 16 g + i][e]: W[16 nt + i][tap][32 kb + 8 g + e], zero padded"""
    N, T, K = w.shape
    KBn, NP = -(-K // 32), -(-N // 64) * 64
    wp = np.zeros((NP, T, KBn * 32), F32)
    wp[:N, :, :K] = w
    return bf16_bits(np.ascontiguousarray(wp.reshape(NP // 16, 16, T, KBn, 4, 8).transpose(0, 2, 3, 4, 1, 5)).reshape(-1))


def pack16_at(w, k):
    """element k of pack16(w) by the index rule alone (the dense loop's statement)"""
    N, T, K = w.shape
    KBn = -(-K // 32)
    e, lane, s = k & 7, (k >> 3) & 63, k >> 9
    kb, tap, nt = s % KBn, (s // KBn) % T, s // (KBn * T)
    n, r = 16 * nt + (lane & 15), 32 * kb + 8 * (lane >> 4) + e
    return w[n, tap, r] if n < N and r < K else F32(0)


def fwd_operand(weight):
    w = np.asarray(weight, F32)
    return bf16(w).transpose(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1])


def bwd_operand(weight, scale=None):
    """rows c, taps in reverse order, reduction o"""
    ws = ws16(weight, scale)
    return ws[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(ws.shape[1], -1, ws.shape[0])


def pack_fwd16(weight):
    return pack16(fwd_operand(weight))


def pack_bwd16(weight, scale=None):
    return pack16(bwd_operand(weight, scale))


# ---- one data-gradient launch ----------------------------------------------------------------------------------------------------------
def dgrad64(ws, stride, g, H, W, adds=(), y=None):
    """ws (O,C,k,k), g (B,O,Ho,Wo), adds [(rule, map)], y (B,C,H,W) or None: bf16-exact values -> dict(t64, S, K, n, blocked)"""
    ws, g = np.asarray(ws, np.float64), np.asarray(g, np.float64)
    O, C, k = ws.shape[0], ws.shape[1], ws.shape[2]
    B = g.shape[0]
    adds = [(rule, np.asarray(r, np.float64)) for rule, r in adds]
    layer = lambda w: dict(weight=w, stride=stride, scale=None)
    with np.errstate(invalid='ignore', over='ignore'):
        t = ref.dx64(layer(ws), g, H, W, adds)
        S = ref.dx64(layer(np.abs(ws)), np.abs(g), H, W, [(rule, np.abs(r)) for rule, r in adds])
    taps = ref.dx64(layer(np.ones((1, 1, k, k))), np.ones((B, 1) + g.shape[2:]), H, W)                      # live taps of every cell
    n = ref.apply_adds(np.zeros((B, 1, H, W)), [(rule, np.ones((B, 1) + r.shape[2:])) for rule, r in adds], np.float64)
    blocked = np.zeros(t.shape, bool) if y is None else np.asarray(y) <= 0
    return dict(t64=t, S=S, K=np.broadcast_to(taps * O, t.shape), n=np.broadcast_to(n, t.shape), blocked=blocked)


def dgrad_bound(d):
    """-> b32 (the float32 value handed to the conversion against t64), b16 (the stored bfloat16 against t64)"""
    b = (d['K'] + d['n'] + 2) * U16 * d['S']
    return b, b + UB * (np.abs(d['t64']) + b)


def dgrad_f32(ws, stride, g, H, W, adds=(), y=None):
    """a float32-accumulate emulation of the launch: products exact, numpy's float32 sums, the adds in order, the mask, one rounding"""
    layer = dict(weight=np.asarray(ws, F32), stride=stride, scale=None)
    t = ref.dx32(layer, np.asarray(g, F32), H, W, [(rule, np.asarray(r, F32)) for rule, r in adds], None if y is None else np.asarray(y, F32))
    return bf16(t)


# ---- one weight gradient ---------------------------------------------------------------------------------------------------------------
def wgrad64(k, stride, scale, x, g, bias=False):
    """x (B,C,H,W), g (B,O,Ho,Wo) bf16-exact; scale (O) float32 or None; bias: the layer has one (an FPN layer, no scale) -> ref.wgrad64's dict"""
    O, C = g.shape[1], x.shape[1]
    out = ref.wgrad64(dict(weight=np.zeros((O, C, k, k), F32), stride=stride, scale=scale), x, g)
    if scale is not None or not bias:
        out['db'], out['S_b'] = None, None
    return out


def wgrad_bound16(wg):
    """(T + 3) 2^-23 |scale[o]| S_W with a scale, (T + 2) 2^-23 S_W without; the bias: (T + 1) 2^-23 S_b"""
    if wg['scale'] is not None:
        return (wg['T'] + 3) * U16 * np.abs(wg['scale'])[:, None, None, None] * wg['S_W'], None
    return (wg['T'] + 2) * U16 * wg['S_W'], None if wg['S_b'] is None else (wg['T'] + 1) * U16 * wg['S_b']


def wgrad_f32(k, stride, scale, x, g):
    """float32-accumulate emulation: cells in ascending order, one rounded add per cell, then the one scale product"""
    cols = tref.columns(np.asarray(x, np.float64), k, stride)
    g2 = np.asarray(g, np.float64).transpose(0, 2, 3, 1)
    T, O = int(np.prod(g2.shape[:3])), g2.shape[3]
    c2, g2 = cols.reshape(T, -1), g2.reshape(T, O)
    acc = np.zeros((O, c2.shape[1]), F32)
    for t in range(T):
        acc = (acc + np.outer(g2[t], c2[t]).astype(F32)).astype(F32)       # a product of two bfloat16 values is exact in float32
    C = x.shape[1]
    dw = acc.reshape(O, k, k, C).transpose(0, 3, 1, 2)
    if scale is not None:
        dw = (dw * np.asarray(scale, F32)[:, None, None, None]).astype(F32)
    return dw

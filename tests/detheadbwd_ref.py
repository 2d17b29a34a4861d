"""numpy restatement of DESIGN.md section 28: the backward of the layers of the detector's heads as the device computes it.  Independent of
the package: nothing here imports cosypose_amd; the forward twin dethead_ref supplies the layers, their GEMM view and the fmaf chain's order.

For one layer (a dict as in dethead_ref) with input x and the gradient g at its PRE-activation output (the shape of the layer's output):
  * dx32: the data gradient as the device computes it, bit for bit: the forward's fmaf chain (accumulator +0.0, blocks of 16 of the REDUCTION
    index -- here the output channel o -- ascending, the taps ascending inside a block, the block's channels in the order 4 g + e) over the
    transposed weight with its taps flipped, rows = g; no bias add.  ConvTranspose2d(2, 2): taps (dy, dx) ascending over g's (2H, 2W) map.
  * dx64: the same sum in float64.
  * wgrad64: dW, db in float64 in torchvision's layout with S_W = sum |g x|, S_b = sum |g| and the term counts T_W, T_b (the cells summed: the
    rows of x; for the deconvolution's bias the rows of g, four times as many).  The device adds T terms in some fixed order, one rounding per
    addition, the products exact inside the fmaf: |dW - dW64| <= (T + 2) 2^-24 S_W and |db - db64| <= (T + 1) 2^-24 S_b.
  * relu_mask: what a row store with the mask writes: y <= 0 ? +0.0 : v (a NaN y passes v) -- torch's threshold_backward.
  * head_backward: a whole head, last layer to first, the masks taken from the float32 forward chain (dethead_ref.layer32).
"""
import numpy as np

import dethead_ref as ref
from frames_ref import fma32

F32 = np.float32
U32 = 2.0 ** -24


def gemm32(rows, w):
    """rows (M, T, K), w (N, T, K) float32 -> (M, N): the kernel's fmaf chain, no bias add"""
    rows, w = np.asarray(rows, F32), np.asarray(w, F32)
    M, T, K = rows.shape
    acc = np.zeros((M, w.shape[0]), F32)
    with np.errstate(invalid='ignore'):
        for k0 in range(0, K, ref.KB32):
            for t in range(T):
                for k in (k0 + 4 * g + e for e in range(4) for g in range(4)):
                    if k < K:
                        acc = fma32(rows[:, t, k][:, None], w[:, t, k][None, :], acc)
    return acc


def dgrad_operands(layer, g):
    """-> rows (M, T, O) of g, the transposed weight (C, T, O), and the function that puts (M, C) back into x's shape"""
    w, kind = np.asarray(layer['weight']), layer['kind']
    if kind == 'linear':
        return g.reshape(g.shape[0], 1, w.shape[0]), w.T.reshape(w.shape[1], 1, w.shape[0]), lambda y: y
    if kind == 'conv':
        O, C, k = w.shape[0], w.shape[1], w.shape[2]
        B, _, H, W = g.shape
        rows = ref.columns(g, k).reshape(B * H * W, k * k, O)                 # tap (ky, kx) of a cell is g at the cell + (ky - 1, kx - 1)
        wt = w[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(C, k * k, O)   # ... which met the weight's tap (2 - ky, 2 - kx) in forward
        return rows, wt, lambda y: y.reshape(B, H, W, C).transpose(0, 3, 1, 2)
    if kind == 'deconv':
        C, O = w.shape[0], w.shape[1]
        B, _, H2, W2 = g.shape
        H, W = H2 // 2, W2 // 2
        rows = g.reshape(B, O, H, 2, W, 2).transpose(0, 2, 4, 3, 5, 1).reshape(B * H * W, 4, O)
        return rows, w.transpose(0, 2, 3, 1).reshape(C, 4, O), lambda y: y.reshape(B, H, W, C).transpose(0, 3, 1, 2)
    raise ValueError(kind)


def dx32(layer, g):
    rows, wt, back = dgrad_operands(layer, np.asarray(g, F32))
    return back(gemm32(rows, wt))


def dx64(layer, g):
    rows, wt, back = dgrad_operands(layer, np.asarray(g, np.float64))
    M, T, O = rows.shape
    return back(rows.reshape(M, T * O) @ wt.astype(np.float64).reshape(-1, T * O).T)


def gemm_columns(layer, g):
    """g in the layer's output shape -> (M, N): one row per cell of x, the GEMM's columns (deconv: (o, dy, dx))"""
    kind = layer['kind']
    if kind == 'linear':
        return g
    B, O = g.shape[:2]
    if kind == 'conv':
        return g.transpose(0, 2, 3, 1).reshape(-1, O)
    H, W = g.shape[2] // 2, g.shape[3] // 2
    return g.reshape(B, O, H, 2, W, 2).transpose(0, 2, 4, 1, 3, 5).reshape(B * H * W, O * 4)


def wgrad64(layer, x, g):
    """-> dict(dW, db, S_W, S_b, T_W, T_b): float64, torchvision's layout (of the twin's layer: siblings are one concatenated weight)"""
    w, kind = np.asarray(layer['weight']), layer['kind']
    rows = ref.as_gemm(layer, np.asarray(x, np.float64))[0]                   # (M, T, C)
    g2 = gemm_columns(layer, np.asarray(g, np.float64))                       # (M, N)
    M, T, C = rows.shape
    r2 = rows.reshape(M, T * C)
    dW, S_W = g2.T @ r2, np.abs(g2).T @ np.abs(r2)                            # (N, T C)
    db, S_b, T_b = g2.sum(0), np.abs(g2).sum(0), M
    if kind == 'conv':
        k = w.shape[2]
        shape = lambda a: a.reshape(w.shape[0], k, k, C).transpose(0, 3, 1, 2)
    elif kind == 'linear':
        shape = lambda a: a
    else:
        O = w.shape[1]
        shape = lambda a: a.reshape(O, 2, 2, C).transpose(3, 0, 1, 2)
        db, S_b, T_b = db.reshape(O, 4).sum(1), S_b.reshape(O, 4).sum(1), 4 * M
    return dict(dW=shape(dW), db=db, S_W=shape(S_W), S_b=S_b, T_W=M, T_b=T_b)


def relu_mask(y, v):
    """y <= 0 ? +0.0 : v; a NaN y passes v"""
    return np.where(np.asarray(y) <= 0, np.zeros_like(v), v)


def head_backward(layers, x, g_out, exact=False):
    """layers one after the other (dethead_ref's lists; the last without a ReLU), g_out at the last layer's output.
    -> dX at x, [wgrad64 dict per layer, first to last].  exact=False: the device's chain (forward dethead_ref.layer32, data gradients
    dx32, masks from the float32 forward's stored values; the weight gradients are the float64 sums over those float32 activations and
    gradients); exact=True: everything in float64 (the host test holds it against torch.autograd)"""
    assert not layers[-1].get('relu'), 'g_out is the pre-activation gradient of the last layer'
    fwd = (lambda l, a: ref.layer64(l, a)[0]) if exact else ref.layer32
    back = dx64 if exact else dx32
    acts = [np.asarray(x, np.float64 if exact else F32)]
    for layer in layers:
        acts.append(fwd(layer, acts[-1]))
    g = np.asarray(g_out, np.float64 if exact else F32)
    grads = [None] * len(layers)
    with np.errstate(invalid='ignore'):
        for i in range(len(layers) - 1, -1, -1):
            grads[i] = wgrad64(layers[i], acts[i], g)                          # g: the pre-activation gradient of layer i
            g = back(layers[i], g)
            if i and layers[i - 1].get('relu'):
                g = relu_mask(acts[i], g)                                      # the launch's own store: layer i - 1's pre-activation gradient
    return g, grads

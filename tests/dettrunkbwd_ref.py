"""numpy restatement of DESIGN.md section 29: the backward of the detector's trunk (ResNet bottlenecks with FrozenBatchNorm, the FPN) as the
device computes it.  Independent of the package: nothing here imports cosypose_amd.  The forward twin dettrunk_ref supplies the layers (dicts:
weight (O,C,k,k), stride, scale or None, bias, relu) and the forward chains, detheadbwd_ref the data gradient's fmaf chain.

"Gradient rows" of a layer are g, the gradient at its PRE-activation value, here as (B,O,Ho,Wo) arrays on the layer's OUTPUT grid.
  * ws: w scale[o], rounded ONCE to float32 (no scale: w); pack_fwd / pack_bwd / pack_bias: the bytes cosy_trunk_weight_pack writes.
  * dx32: dX on the (H, W) grid, bit for bit: section 28's chain over ws (blocks of 16 o ascending, the flipped taps ascending inside a block, every
    term one fmaf).  At stride 2 the chain runs over g spread onto the even cells of the (H, W) grid with +0.0 between them: a dead tap then
    contributes fma(+0.0, ws, acc) = acc, the bits of skipping it (finite weights).  Then the store: the add operands in order
    (SAME / EVEN / NEAREST_T), the ReLU mask y <= 0 ? +0.0 : t.
  * dx64: the same in float64.  wgrad64: dW = scale[o] sum g x in float64 with S_W = sum |g x| (unscaled), db, S_b and the term count T.
  * block_backward, fpn_backward, trunk_backward: the chains of section 29 over dettrunk_ref's forward with its kept intermediates.
"""
import numpy as np

import detheadbwd_ref as bref
import dettrunk_ref as tref

F32 = np.float32
U32 = 2.0 ** -24
SAME, EVEN, NEAREST_T = 'same', 'even', 'nearest_t'


def ws_of(layer, exact=False):
    """w scale[o]: one rounded float32 product per element (exact: the float64 product)"""
    w = np.asarray(layer['weight'])
    if exact:
        w = w.astype(np.float64)
        return w if layer.get('scale') is None else w * np.asarray(layer['scale'], np.float64)[:, None, None, None]
    w = w.astype(F32)
    return w if layer.get('scale') is None else (w * np.asarray(layer['scale'], F32)[:, None, None, None]).astype(F32)


def pack(w):
    """(N, taps, K) float32 -> the fragment order of cosy_head_conv: [N_pad / 16][tap][k-block][lane = 16 g + i][e], zero padded"""
    N, T, K = w.shape
    KBn, NP = -(-K // 16), -(-N // 64) * 64
    wp = np.zeros((NP, T, KBn * 16), F32)
    wp[:N, :, :K] = w
    return np.ascontiguousarray(wp.reshape(NP // 16, 16, T, KBn, 4, 4).transpose(0, 2, 3, 4, 1, 5)).reshape(-1)


def pack_fwd(layer):
    w = np.asarray(layer['weight'], F32)
    return pack(w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1]))


def pack_bwd(layer):
    ws = ws_of(layer)
    return pack(ws[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(ws.shape[1], -1, ws.shape[0]))


def pack_bias(layer):
    b = np.asarray(layer['bias'], F32)
    out = np.zeros(-(-b.shape[0] // 64) * 64, F32)
    out[:b.shape[0]] = b
    return out


def spread(g, H, W, stride):
    """g (B,O,Ho,Wo) -> (B,O,H,W): g at the cells (stride y, stride x), +0.0 elsewhere"""
    if stride == 1:
        assert g.shape[2:] == (H, W), (g.shape, H, W)
        return g
    B, O, Ho, Wo = g.shape
    assert (Ho, Wo) == (tref.out_size(H, 2), tref.out_size(W, 2)), (g.shape, H, W)
    z = np.zeros((B, O, H, W), g.dtype)
    z[:, :, 0:2 * Ho:2, 0:2 * Wo:2] = g
    return z


def nearest_t_cells(n_coarse, n_fine):
    """for every coarse index the finer indices whose section 27 source it is: contiguous ranges [lo, hi)"""
    src = tref.nearest_index(n_coarse, n_fine)
    return [(int(np.searchsorted(src, c, 'left')), int(np.searchsorted(src, c, 'right'))) for c in range(n_coarse)]


def apply_adds(t, adds, dtype):
    """the store's add operands, in order, one rounded add each"""
    t = t.copy()
    H, W = t.shape[2:]
    with np.errstate(invalid='ignore', over='ignore'):
        for rule, r in adds:
            r = np.asarray(r, dtype)
            if rule == SAME:
                assert r.shape == t.shape
                t = (t + r).astype(dtype)
            elif rule == EVEN:
                assert r.shape[2:] == (tref.out_size(H, 2), tref.out_size(W, 2)), (r.shape, t.shape)
                t[:, :, ::2, ::2] = (t[:, :, ::2, ::2] + r).astype(dtype)          # every other cell untouched: a -0.0 stays
            elif rule == NEAREST_T:
                sy, sx = tref.nearest_index(H, r.shape[2]), tref.nearest_index(W, r.shape[3])
                for fy in range(r.shape[2]):                                       # ascending (fy, fx): a coarse cell meets its finer cells in that order
                    for fx in range(r.shape[3]):
                        t[:, :, sy[fy], sx[fx]] = (t[:, :, sy[fy], sx[fx]] + r[:, :, fy, fx]).astype(dtype)
            else:
                raise ValueError(rule)
    return t


def _dx(layer, g, H, W, adds, y, exact):
    dtype = np.float64 if exact else F32
    g = np.asarray(g, dtype)
    k, stride = layer['weight'].shape[2], layer.get('stride', 1)
    if k == 1 and stride == 2:
        raise ValueError('a 1x1 at stride 2 is a stride-1 data gradient on its OUTPUT grid whose rows enter through EVEN')
    conv = dict(kind='conv', weight=ws_of(layer, exact))
    t = np.ascontiguousarray((bref.dx64 if exact else bref.dx32)(conv, spread(g, H, W, stride)))
    t = apply_adds(t.astype(dtype), adds, dtype)
    if y is not None:
        t = bref.relu_mask(y, t)
    return t


def dx32(layer, g, H, W, adds=(), y=None):
    return _dx(layer, g, H, W, adds, y, False)


def dx64(layer, g, H, W, adds=(), y=None):
    return _dx(layer, g, H, W, adds, y, True)


def on_output_grid(layer):
    """downsample.0 for its data gradient: the same 1x1 at stride 1 on the (Ho, Wo) grid"""
    return dict(layer, stride=1)


def wgrad64(layer, x, g):
    """-> dict(dW (scaled, float64, (O,C,k,k)), S_W (sum |g x|, unscaled), db, S_b (None with a scale), T, scale)"""
    w = np.asarray(layer['weight'])
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    cols = tref.columns(np.asarray(x, np.float64), k, layer.get('stride', 1))      # (B,Ho,Wo,kk,C)
    g2 = np.asarray(g, np.float64).transpose(0, 2, 3, 1)                             # (B,Ho,Wo,O)
    assert cols.shape[:3] == g2.shape[:3], (cols.shape, g2.shape)
    T = int(np.prod(g2.shape[:3]))
    with np.errstate(invalid='ignore'):
        c2, g2 = cols.reshape(T, k * k * C), g2.reshape(T, O)
        dW, S = g2.T @ c2, np.abs(g2).T @ np.abs(c2)
    shape = lambda a: a.reshape(O, k, k, C).transpose(0, 3, 1, 2)
    out = dict(dW=shape(dW), S_W=shape(S), db=None, S_b=None, T=T, scale=None)
    if layer.get('scale') is not None:
        out['scale'] = np.asarray(layer['scale'], np.float64)
        out['dW'] = out['dW'] * out['scale'][:, None, None, None]
    else:
        out['db'], out['S_b'] = g2.sum(0), np.abs(g2).sum(0)
    return out


def wgrad_bound(wg):
    """the tests' bounds: (T + 3) u |scale[o]| S_W with a scale, (T + 2) u S_W without; the bias: (T + 1) u S_b"""
    if wg['scale'] is not None:
        return (wg['T'] + 3) * U32 * np.abs(wg['scale'])[:, None, None, None] * wg['S_W'], None
    return (wg['T'] + 2) * U32 * wg['S_W'], (wg['T'] + 1) * U32 * wg['S_b']


# ---- the forward with everything the backward reads -----------------------------------------------------------------------------------------------
def forward_keep(net, images, exact=False):
    """-> dict: (stage, i) from 1 -> dict(x, a, b, out) of every block, 'feats', 'inner', 'out' (the four maps and pool)"""
    if exact:
        f = lambda layer, x, r=None: tref.layer64(layer, x, r)[0]
        images = np.asarray(images, np.float64)
    else:
        f = tref.layer32
        images = np.asarray(images, F32)
    keep = {}
    v = tref.maxpool(f(net['stem'], tref.stem_columns(images)))
    keep['pooled'] = v
    feats = []
    for s, blocks in enumerate(net['stages'], 1):
        for i, blk in enumerate(blocks):
            a = f(blk['conv1'], v)
            b = f(blk['conv2'], a)
            short = v if blk.get('down') is None else f(blk['down'], v)
            out = f(blk['conv3'], b, short)
            keep[(s, i)] = dict(x=v, a=a, b=b, out=out)
            v = out
        feats.append(v)
    L = len(feats)
    inner = [None] * L
    for l in range(L - 1, -1, -1):
        inner[l] = f(net['inner'][l], feats[l], None if l == L - 1 else inner[l + 1])
    outs = [f(net['outer'][l], inner[l]) for l in range(L)]
    keep.update(feats=feats, inner=inner, out=outs + [np.ascontiguousarray(outs[-1][..., ::2, ::2])])
    return keep


def fpn_backward(net, keep, g_out, exact=False):
    """g_out: the gradients at the four output maps (pool's already added into the last).  Bottom-up.
    -> params {name: wgrad64 dict}, G_inner [per level]"""
    dx = dx64 if exact else dx32
    params, G = {}, []
    for l, g in enumerate(g_out):
        H, W = keep['inner'][l].shape[2:]
        params[f'fpn.layer_blocks.{l}'] = wgrad64(net['outer'][l], keep['inner'][l], g)
        G.append(dx(net['outer'][l], g, H, W, [] if l == 0 else [(NEAREST_T, G[l - 1])]))
        params[f'fpn.inner_blocks.{l}'] = wgrad64(net['inner'][l], keep['feats'][l], G[l])
    return params, G


def block_backward(blk, k, g3, adds_tail=(), need_dx=True, mask_dx=True, exact=False):
    """one bottleneck from g3 = mask(out) G.  k: dict(x, a, b, out) of forward.  adds_tail: the operands listed AFTER the shortcut's (the FPN's).
    -> wgrad dicts {conv1, conv2, conv3 (, downsample.0)}, rows dict(g1, g2, g3 (, down_dx)), the launch's store for the block below (or None)"""
    dx = dx64 if exact else dx32
    H, W = k['x'].shape[2:]
    Ho, Wo = k['b'].shape[2:]
    stride = blk['conv2'].get('stride', 1)
    g2 = dx(blk['conv3'], g3, Ho, Wo, y=k['b'])
    g1 = dx(blk['conv2'], g2, H, W, y=k['a'])
    params = dict(conv3=wgrad64(blk['conv3'], k['b'], g3), conv2=wgrad64(blk['conv2'], k['a'], g2), conv1=wgrad64(blk['conv1'], k['x'], g1))
    rows = dict(g1=g1, g2=g2, g3=g3)
    if blk.get('down') is not None:
        params['downsample.0'] = wgrad64(blk['down'], k['x'], g3)
    below = None
    if need_dx:
        if blk.get('down') is None:
            adds = [(SAME, g3)]
        else:
            rows['down_dx'] = dx(on_output_grid(blk['down']), g3, Ho, Wo)
            adds = [(EVEN if stride == 2 else SAME, rows['down_dx'])]
        below = dx(blk['conv1'], g1, H, W, adds + list(adds_tail), y=k['x'] if mask_dx else None)
    return params, rows, below


def trunk_backward(net, images, grads, train_from_stage=2, exact=False, input_grad=False, keep=None):
    """grads: the gradients at the maps ['0', '1', '2', '3'] and optionally 'pool' (None: zeros).
    -> dict(params={torchvision's name without '.weight': wgrad64 dict}, rows={name: gradient rows as (B,C,H,W)}, dx=the gradient at the first
    trainable block's input through that block alone (input_grad; unmasked, without the FPN's lateral), keep=the forward's intermediates)"""
    keep = forward_keep(net, images, exact) if keep is None else keep
    dtype = np.float64 if exact else F32
    dx = dx64 if exact else dx32
    L = len(net['stages'])
    if not 1 <= train_from_stage <= L + 1:
        raise ValueError(f'train_from_stage must lie in [1, {L + 1}]')
    g_out = [np.zeros(keep['out'][l].shape, dtype) if grads[l] is None else np.asarray(grads[l], dtype) for l in range(L)]
    if len(grads) > L and grads[L] is not None:
        z = np.zeros_like(g_out[-1])
        z[..., ::2, ::2] = np.asarray(grads[L], dtype)
        with np.errstate(invalid='ignore'):
            g_out[-1] = (g_out[-1] + z).astype(dtype)
    params, G = fpn_backward(net, keep, g_out, exact)
    rows = {f'fpn.G_inner.{l}': G[l] for l in range(L)}
    result = dict(params=params, rows=rows, dx=None, keep=keep)

    def lateral(s, masked):
        H, W = keep['feats'][s - 1].shape[2:]
        r = dx(net['inner'][s - 1], G[s - 1], H, W, y=keep['feats'][s - 1] if masked else None)
        rows[f'fpn.lateral_dx.{s - 1}'] = r
        return r
    g3 = None
    for s in range(L, train_from_stage - 1, -1):
        blocks = net['stages'][s - 1]
        if s == L:
            g3 = lateral(s, True)
        for i in range(len(blocks) - 1, -1, -1):
            first = s == train_from_stage and i == 0
            tail = []
            if i == 0 and not first:
                tail = [(SAME, lateral(s - 1, False))]
            p, r, below = block_backward(blocks[i], keep[(s, i)], g3, tail, need_dx=not first or input_grad, mask_dx=not first, exact=exact)
            name = f'body.layer{s}.{i}'
            params.update({f'{name}.{k}': v for k, v in p.items()})
            rows.update({f'{name}.{k}': v for k, v in r.items()})
            if first:
                result['dx'] = below
            g3 = below
    return result

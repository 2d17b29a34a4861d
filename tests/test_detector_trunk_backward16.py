"""The backward of the detector's trunk on bfloat16 rows on the GPU (csrc/kernels_detbwd16.hip behind cosypose_amd/detector_trunk_backward.py,
DESIGN.md section 30) against the CPU twin tests/dettrunkbwd16_ref.py, which test_detector_trunk_backward16_host.py holds against torch.

Criteria.  The order of the 32 additions inside a 16-bit MFMA is the hardware's: nothing but the packings and device against device is
bit-equal.  Every numeric check is ONE launch against float64 on that launch's own operands as the device holds them (bf16-exact values).
Data gradient, per stored element: t64 = accumulate, then the adds; S = sum |ws g| + sum |add terms|; K = live taps x o summed; n = add terms
taken; the float32 value handed to the conversion lies within b = (K + n + 2) 2^-23 S of t64, the stored bfloat16 within b + 2^-8 (|t64| + b);
where the mask blocks, exactly +0.0.  Weight gradient: |dW - dW64| <= (T + 3) 2^-23 |scale[o]| S_W, (T + 2) 2^-23 S_W without a scale,
(T + 1) 2^-23 S_b for a bias.  Two calls give equal bits.  Every test prints its largest error as a share of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import dettrunk_case as tc
import dettrunkbwd_case as bc
import dettrunkbwd16_ref as r16
from cosypose_amd import Detector, DetectorTrunk, TrainableTrunkLayer, TrunkLayer, layer_dgrad, layer_wgrad
from cosypose_amd import _lib, detector_trunk_backward as tb
from cosypose_amd.detector_heads import TrainableLayer, pack_weight

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
RULES = {r16.SAME: _lib.TRUNK_ADD_SAME, r16.EVEN: _lib.TRUNK_ADD_EVEN, r16.NEAREST_T: _lib.TRUNK_ADD_NEAREST_T}
RESIZE = (48, 64)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    t = t.detach()
    return (t.float() if t.dtype == BF16 else t).cpu().numpy()


def bits16(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def trainable16(layer, name='layer'):
    """a twin layer dict as a bfloat16 TrainableTrunkLayer: a FrozenBatchNorm with variance 1 and mean 0 gives exactly the scale and the shift"""
    O = layer['weight'].shape[0]
    w = torch.from_numpy(layer['weight'])
    if layer['scale'] is None:
        return TrainableTrunkLayer(name, w, bias=torch.from_numpy(layer['bias']), stride=layer['stride'], relu=layer['relu'], device='cuda', dtype=BF16)
    bn = (torch.from_numpy(layer['scale']), torch.from_numpy(layer['bias']), torch.zeros(O), torch.ones(O))
    return TrainableTrunkLayer(name, w, bn=bn, stride=layer['stride'], relu=layer['relu'], device='cuda', dtype=BF16)


def make_layer(rng, k, stride, ci, co, scaled=True):
    w = (rng.normal(0, 1, (co, ci, k, k)) / np.sqrt(ci * k * k)).astype(F32)
    scale = None
    if scaled:
        scale = rng.uniform(0.5, 1.5, co).astype(F32) * rng.choice([-1, 1], co).astype(F32)
        if scaled == 'negative':
            scale = -np.abs(scale)
    return dict(weight=w, stride=stride, scale=scale, bias=rng.normal(0, 0.5, co).astype(F32), relu=True)


def check_dgrad(name, got, d, quiet=False):
    """got: the stored rows as float32 (B,C,H,W); d: the twin's dgrad64 of this launch -> the largest share of the bound used"""
    _, b16 = r16.dgrad_bound(d)
    want, blocked = d['t64'], d['blocked']
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not got[blocked].any() and not np.signbit(got[blocked]).any(), (name, 'a blocked element is not +0.0')
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got) & ~blocked, nan & ~blocked), (name, 'the NaNs are not where the twin has them')
    ok = ~blocked & ~nan
    err = np.abs(got.astype(np.float64)[ok] - want[ok])
    share = float((err / np.maximum(b16[ok], 1e-300)).max()) if err.size else 0.0
    if not quiet:
        print(f'{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest share of the bound = {share:.3f}, blocked {int(blocked.sum())} of {blocked.size}')
    assert (err <= b16[ok]).all(), (name, share)
    return share


def check_wgrad(name, got, wg, quiet=False):
    """got: [dW (, db)] from the device; wg: the twin's wgrad64 dict -> the largest share of a bound used"""
    bw, bb = r16.wgrad_bound16(wg)
    worst = 0.0
    assert (len(got) == 2) == (wg['db'] is not None), name
    for which, g, want, bound in (('dW', got[0], wg['dW'], bw),) + ((('db', got[1], wg['db'], bb),) if wg['db'] is not None else ()):
        g = host(g)
        assert g.shape == want.shape and g.dtype == F32, (name, which, g.shape, want.shape, g.dtype)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan), (name, which, 'the NaNs are not where the twin has them')
        err = np.where(nan, 0.0, np.abs(g.astype(np.float64) - np.where(nan, 0.0, want)))
        share = float((err / np.maximum(np.where(nan, 1.0, bound), 1e-300)).max()) if err.size else 0.0
        worst = max(worst, share)
        if not quiet:
            print(f'{name} {which}: max |err| = {float(err.max()):.3e}, largest share of the bound (T = {wg["T"]}) = {share:.3f}')
        assert (err <= np.where(nan, 0.0, bound)).all(), (name, which, share)
    return worst


# ---- packings ----------------------------------------------------------------------------------------------------------------------------
PACKS = [('3x3-negative-scale', 3, 8, 24, 'negative'), ('1x1-fpn', 1, 40, 72, False), ('3x3-72-40', 3, 72, 40, True), ('1x1-24-8', 1, 24, 8, True),
         ('3x3-40-72-fpn', 3, 40, 72, False), ('1x1-8-40', 1, 8, 40, 'negative')]


@pytest.mark.parametrize('c', PACKS, ids=lambda c: c[0])
def test_the_device_pack_writes_the_twins_bytes(c):
    name, k, ci, co, scaled = c
    layer = make_layer(np.random.RandomState(ci * 7 + co + k), k, 1, ci, co, scaled)
    tl = trainable16(layer).refresh()
    w = layer['weight']
    assert tl.w.dtype == BF16 and tl.w_t.dtype == BF16 and tl.bias.dtype == torch.float32 and tl.weight.dtype == torch.float32
    host_pack = pack_weight(torch.from_numpy(w).permute(0, 2, 3, 1).reshape(co, k * k, ci), BF16)
    assert np.array_equal(bits16(tl.w), bits16(host_pack)), 'fwd: the host packing of the weight rounded to bfloat16'
    assert np.array_equal(bits16(tl.w), r16.pack_fwd16(w))
    assert np.array_equal(bits16(tl.w_t), r16.pack_bwd16(w, layer['scale'])), 'bwd: the twin\'s rule over ws rounded once'
    bias = np.zeros(-(-co // 64) * 64, F32)
    bias[:co] = layer['bias']
    assert np.array_equal(bits(host(tl.bias)), bits(bias))
    again = trainable16(layer).refresh()
    assert torch.equal(tl.w.view(torch.int16), again.w.view(torch.int16)) and torch.equal(tl.w_t.view(torch.int16), again.w_t.view(torch.int16))


def test_the_gradient_pack_rounds_to_nearest_even():
    rng = np.random.RandomState(2)
    for B, C, H, W in ((2, 24, 5, 7), (1, 8, 1, 1), (3, 72, 2, 1)):
        g = rng.normal(0, 1, (B, C, H, W)).astype(F32)
        g.reshape(-1)[:4] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, np.inf]
        rows = torch.full((B * H * W, C), 7.0, dtype=BF16, device='cuda')
        tb.trunk_grad_pack(dev(g), rows, B, C, H * W)
        want = r16.bf16_bits(g.transpose(0, 2, 3, 1).reshape(-1, C)).reshape(-1)
        assert np.array_equal(bits16(rows), want)
        tb.trunk_grad_pack(None, rows, B, C, H * W)
        assert not bits16(rows).any()                                         # a null gradient is +0.0 everywhere


# ---- single data-gradient launches ---------------------------------------------------------------------------------------------------------
def dgrad_case16(c):
    """bc.dgrad_data's operands rounded to bfloat16: what the device holds"""
    layer, g, ops, y = bc.dgrad_data(c)
    return layer, r16.bf16(g), [(rule, r16.bf16(m)) for rule, m in ops], None if y is None else r16.bf16(y)


@pytest.mark.parametrize('c', bc.DGRAD, ids=bc.case_id)
def test_a_data_gradient_launch_meets_its_bound(c):
    layer, g, ops, y = dgrad_case16(c)
    H, W = c[5][1:]
    tl = trainable16(layer)
    call = lambda: layer_dgrad(tl, dev(g), H, W, [(RULES[r], dev(m)) for r, m in ops], None if y is None else dev(y))
    got = call()
    d = r16.dgrad64(r16.ws16(layer['weight'], layer['scale']), layer['stride'], g, H, W, ops, y)
    check_dgrad(c[0], host(got), d)
    assert r16.is_bf16(host(got)[np.isfinite(host(got))])
    assert torch.equal(got.view(torch.int32), call().view(torch.int32))
    if y is not None:                                         # a stored y of exactly 0 (or -0.0) blocks its element: +0.0, whatever arrives
        blocked = host(got)[y == 0]
        assert blocked.size and not blocked.any() and not np.signbit(blocked).any()


@pytest.mark.parametrize('c', bc.EVEN_CASES, ids=bc.case_id)
def test_a_strided_1x1_enters_through_the_even_rule_and_an_odd_cell_is_left_untouched(c):
    # bc.even_data's shapes with plain values: its planted 1e-20 x 1e-30 products underflow, and section 30's bound takes products for exact
    B, H, W = c[1]
    rng = np.random.RandomState(H * 8 + W)
    down, conv1 = make_layer(rng, 1, 2, 8, 16), make_layer(rng, 1, 1, 8, 16)
    g3 = r16.bf16(rng.normal(0, 1, (B, 16, (H - 1) // 2 + 1, (W - 1) // 2 + 1)).astype(F32))
    g1 = r16.bf16(rng.normal(0, 1, (B, 16, H, W)).astype(F32))
    td, t1 = trainable16(down), trainable16(conv1)
    d_rows = layer_dgrad(td, dev(g3), *g3.shape[2:], stride=1)
    dd = r16.dgrad64(r16.ws16(down['weight'], down['scale']), 1, g3, *g3.shape[2:])
    check_dgrad(c[0] + ' on the output grid', host(d_rows), dd)
    got = host(layer_dgrad(t1, dev(g1), H, W, [(_lib.TRUNK_ADD_EVEN, d_rows)]))
    d1 = r16.dgrad64(r16.ws16(conv1['weight'], conv1['scale']), 1, g1, H, W, [(r16.EVEN, host(d_rows))])
    check_dgrad(c[0], got, d1)
    plain = host(layer_dgrad(t1, dev(g1), H, W))                               # the same launch without the operand: device against device
    odd = np.ones((H, W), bool)
    odd[::2, ::2] = False
    assert np.array_equal(bits(got[:, :, odd]), bits(plain[:, :, odd])) and (d1['n'][:, :, odd] == 0).all() and (d1['n'][:, :, ~odd] == 1).all()
    if (~odd).sum():
        assert (bits(got[:, :, ~odd]) != bits(plain[:, :, ~odd])).any()


def test_a_nan_reaches_exactly_its_receptive_field():
    c = next(x for x in bc.DGRAD if x[0] == 'd-s1-k3-c40-24-5x7-same-mask')
    layer, g, ops, _ = dgrad_case16(c)
    g = g.copy()
    g[0, 3, 2, 3] = np.nan
    tl = trainable16(layer)
    got = host(layer_dgrad(tl, dev(g), 5, 7, [(RULES[r], dev(m)) for r, m in ops]))
    want = np.zeros(got.shape, bool)
    want[0, :, 1:4, 2:5] = True
    assert np.array_equal(np.isnan(got), want)
    check_dgrad('a NaN in g', got, r16.dgrad64(r16.ws16(layer['weight'], layer['scale']), 1, g, 5, 7, ops))
    c2 = next(x for x in bc.DGRAD if x[0] == 'd-s2-k3-c8-24-5x7')                 # stride 2: the output cell (1, 1) meets the input cells (1..3, 1..3)
    layer, g, ops, _ = dgrad_case16(c2)
    g = g.copy()
    g[1, 0, 1, 1] = np.nan
    got = host(layer_dgrad(trainable16(layer), dev(g), 5, 7))
    want = np.zeros(got.shape, bool)
    want[1, :, 1:4, 1:4] = True
    assert np.array_equal(np.isnan(got), want)


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------------
# (name, ksize, stride, C_in, C_out, (B, H, W) of x, scale: True, False (an FPN layer: a bias gradient) or 'negative')
TS = (31, 32, 33, 255, 256, 257, 515)                                              # one k-step of 32 cells, the slab edge, three slabs
WGRAD = [(f'w-s1-k1-c24-T{T}', 1, 1, 24, 24, (1, 1, T), True) for T in TS]
WGRAD += [(f'w-s2-k3-c8-T{T}', 3, 2, 8, 24, (1, 2, 2 * T - 1), True) for T in TS]
WGRAD += [(f'w-s1-k3-one-cell-wide-T{T}', 3, 1, 8, 24, (1, T, 1), False) for T in (33, 257)]     # every horizontal tap is outside
WGRAD += [(f'w-s{s}-k{k}-c40-{H}x{W}', k, s, 40, 24, (2, H, W), True) for k in (3, 1) for s in (1, 2) for H, W in bc.MAPS]
WGRAD += [(f'w-k{k}-c{ci}-5x7', k, 1, ci, 40, (2, 5, 7), True) for k in (3, 1) for ci in (8, 24, 72)]
WGRAD += [('w-negative-scale', 3, 2, 8, 24, (2, 5, 7), 'negative'), ('w-fpn-k3-bias', 3, 1, 16, 16, (2, 5, 7), False), ('w-fpn-k1-bias', 1, 1, 72, 16, (2, 4, 6), False),
          ('w-s2-k1-c72-bias-off', 1, 2, 72, 40, (2, 5, 7), 'negative')]


def wgrad_data16(c):
    name, k, stride, ci, co, (B, H, W), scaled = c
    rng = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31))
    layer = make_layer(rng, k, stride, ci, co, scaled)
    x = r16.bf16(rng.normal(0, 1, (B, ci, H, W)).astype(F32))
    g = r16.bf16(rng.normal(0, 1, (B, co, (H - 1) // stride + 1, (W - 1) // stride + 1)).astype(F32))
    return layer, x, g


@pytest.mark.parametrize('c', WGRAD, ids=lambda c: c[0])
def test_a_weight_gradient_meets_the_float64_bound(c):
    layer, x, g = wgrad_data16(c)
    tl = trainable16(layer)
    got = layer_wgrad(tl, dev(x), dev(g))
    wg = r16.wgrad64(c[1], c[2], layer['scale'], x, g, bias=layer['scale'] is None)
    assert wg['T'] == g.shape[0] * g.shape[2] * g.shape[3]
    check_wgrad(c[0], got, wg)
    again = layer_wgrad(tl, dev(x), dev(g))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))
    assert tuple(got[0].shape) == layer['weight'].shape and got[0].dtype == torch.float32
    if c[6] == 'negative':
        assert (layer['scale'] < 0).all()


def test_the_slabs_sit_where_the_cases_expect_them():
    slab = _lib.lib().cosy_head_wgrad_slab_rows
    assert [slab(t) for t in TS] == [256] * len(TS) and -(-515 // 256) == 3


# ---- the whole trunk -----------------------------------------------------------------------------------------------------------------------
def nchw(rows, B, h, w):
    return host(rows.view(B, h, w, -1).permute(0, 3, 1, 2).contiguous())


def twin_of(layer):
    """what one launch needs of a TrainableTrunkLayer: ws as the device packs it, the scale, the kernel size and the stride"""
    scale = None if layer.scale is None else host(layer.scale)[:layer.c_out]
    return dict(ws=r16.ws16(host(layer.weight), scale), scale=scale, k=layer.ksize, stride=layer.stride, bias=layer.bias_param is not None, name=layer.name)


def run_trunk16(trunk, shape, grads):
    """forward + backward through the four maps -> the maps, {parameter: grad}, the captured gradient rows, the kept rows"""
    trunk.zero_grad()
    trunk.keep_rows = True
    out = trunk(dev(tc.trunk_images(shape)))
    keep = out[0].grad_fn.keep
    torch.autograd.backward(out[:4], [dev(g) for g in grads[:4]])
    return out, {k: p.grad.clone() for k, p in trunk.named_parameters()}, {k: nchw(*v) for k, v in trunk.last_rows.items()}, keep


def launches(trunk, keep, rows, grads):
    """the launches of detector_trunk_backward.backward, each with its own operands as the device held them:
    ('d', name of the output buffer, layer, g, (H, W), adds, y, stride) and ('w', layer, x, g)"""
    B, feats, starts = keep['B'], keep['feats'], keep['starts']
    L, tfs = len(trunk.stages), trunk.train_from_stage
    kept = lambda t, h, w: nchw(t, B, h, w)
    inner = [kept(keep['inner'][starts[l]:starts[l + 1]], feats[l][1], feats[l][2]) for l in range(L)]
    feat = [kept(*feats[l]) for l in range(L)]
    out = []
    for l in range(L):
        _, h, w = feats[l]
        g = r16.bf16(grads[l])
        out.append(('w', trunk.outer[l], inner[l], g))
        out.append(('d', f'fpn.G_inner.{l}', trunk.outer[l], g, (h, w), [] if l == 0 else [(r16.NEAREST_T, rows[f'fpn.G_inner.{l - 1}'])], None, 1))
        out.append(('w', trunk.inner[l], feat[l], rows[f'fpn.G_inner.{l}']))

    def lateral(s, masked):
        _, h, w = feats[s - 1]
        out.append(('d', f'fpn.lateral_dx.{s - 1}', trunk.inner[s - 1], rows[f'fpn.G_inner.{s - 1}'], (h, w), [], feat[s - 1] if masked else None, 1))
        return rows[f'fpn.lateral_dx.{s - 1}']
    for s in range(L, tfs - 1, -1):
        blocks = trunk.stages[s - 1]
        if s == L:
            lateral(s, True)
        for i in range(len(blocks) - 1, -1, -1):
            blk, k = blocks[i], keep['blocks'][(s, i)]
            H, W, Ho, Wo = k['H'], k['W'], k['Ho'], k['Wo']
            name = f'body.layer{s}.{i}'
            x, a, b = kept(k['x'], H, W), kept(k['a'], H, W), kept(k['b'], Ho, Wo)
            g3, g2, g1 = rows[f'{name}.g3'], rows[f'{name}.g2'], rows[f'{name}.g1']
            out.append(('d', f'{name}.g2', blk.conv3, g3, (Ho, Wo), [], b, 1))
            out.append(('d', f'{name}.g1', blk.conv2, g2, (H, W), [], a, blk.conv2.stride))
            out += [('w', blk.conv3, b, g3), ('w', blk.conv2, a, g2), ('w', blk.conv1, x, g1)]
            if blk.downsample is not None:
                out.append(('w', blk.downsample, x, g3))
            if s == tfs and i == 0:
                break
            tail = [(r16.SAME, lateral(s - 1, False))] if i == 0 else []
            if blk.downsample is None:
                adds = [(r16.SAME, g3)]
            else:
                out.append(('d', f'{name}.down_dx', blk.downsample, g3, (Ho, Wo), [], None, 1))
                adds = [(r16.EVEN if blk.conv2.stride == 2 else r16.SAME, rows[f'{name}.down_dx'])]
            below = f'body.layer{s}.{i - 1}.g3' if i else f'body.layer{s - 1}.{len(trunk.stages[s - 2]) - 1}.g3'
            out.append(('d', below, blk.conv1, g1, (H, W), adds + tail, x, 1))
    return out


def check_launches(name, trunk, keep, rows, grads, pgrads):
    seen_rows, seen_params, worst_d, worst_w = set(), set(), 0.0, 0.0
    for item in launches(trunk, keep, rows, grads):
        if item[0] == 'd':
            _, out_name, layer, g, (H, W), adds, y, stride = item
            t = twin_of(layer)
            d = r16.dgrad64(t['ws'], stride, g, H, W, adds, y)
            worst_d = max(worst_d, check_dgrad(out_name, rows[out_name], d, quiet=True))
            seen_rows.add(out_name)
        else:
            _, layer, x, g = item
            t = twin_of(layer)
            wg = r16.wgrad64(t['k'], t['stride'], t['scale'], x, g, bias=t['bias'])
            got = [pgrads[f'{t["name"]}.weight']] + ([pgrads[f'{t["name"]}.bias']] if t['bias'] else [])
            worst_w = max(worst_w, check_wgrad(t['name'], got, wg, quiet=True))
            seen_params |= {f'{t["name"]}.weight'} | ({f'{t["name"]}.bias'} if t['bias'] else set())
    top = f'body.layer{len(trunk.stages)}.{len(trunk.stages[-1]) - 1}.g3'             # the masked lateral's buffer under its second name
    assert seen_rows | ({top} if top in rows else set()) == set(rows), (sorted(set(rows) - seen_rows), sorted(seen_rows - set(rows)))
    assert seen_params == set(pgrads)
    print(f'{name}: {len(seen_rows)} data-gradient launches, largest share of a bound = {worst_d:.3f}; {len(seen_params)} parameter gradients, largest share = {worst_w:.3f}')
    return worst_d, worst_w


@pytest.mark.parametrize('shape', tc.INPUTS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('tfs', bc.TRAIN_FROM)
def test_every_launch_of_the_trunks_backward_meets_its_bound(shape, tfs):
    sd = bc.torch_sd()
    trunk = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=tfs, train_dtype=BF16)
    assert trunk.train_dtype == BF16 and all(p.dtype == torch.float32 for p in trunk.parameters())
    grads = bc.trunk_grads(shape)
    out, pgrads, rows, keep = run_trunk16(trunk, shape, grads)
    plain = DetectorTrunk.from_state_dict(sd, dtype=BF16, device='cuda')
    with torch.no_grad():
        for l, (o, w) in enumerate(zip(out, plain(dev(tc.trunk_images(shape))))):    # the same kernels over the same bytes
            assert o.dtype == torch.float32 and torch.equal(o.view(torch.int32), w.view(torch.int32)), f'forward map {l}'
    assert set(rows) == {k for k in bc.trunk_want(shape)['rows'] if bc.trained(k, tfs)}
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in pgrads.values())
    assert all(t.dtype == BF16 for t in [keep['inner']] + [f[0] for f in keep['feats']] + [k[n] for k in keep['blocks'].values() for n in ('x', 'a', 'b', 'out')])
    check_launches(f'train_from_stage={tfs}', trunk, keep, rows, grads, pgrads)
    _, again, rows2, _ = run_trunk16(trunk, shape, grads)                  # two calls give equal bits
    assert all(torch.equal(pgrads[k].view(torch.int32), again[k].view(torch.int32)) for k in pgrads)
    assert all(np.array_equal(bits(rows[k]), bits(rows2[k])) for k in rows)
    kept16 = trunk.last_kept_bytes
    full = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=tfs)
    full(dev(tc.trunk_images(shape)))
    print(f'kept bytes: bfloat16 {kept16}, float32 {full.last_kept_bytes}: {kept16 / full.last_kept_bytes:.3f}')
    assert 0 < kept16 <= 0.55 * full.last_kept_bytes


def test_an_sgd_step_moves_the_float32_masters_and_the_next_forward_repacks():
    shape = tc.INPUTS[0]
    trunk = DetectorTrunk.from_state_dict(bc.torch_sd(), device='cuda', trainable=True, train_dtype=BF16)
    n_layers = sum(hasattr(l, 'weight') for l in trunk.layers())
    assert trunk.pack_count == 0
    run_trunk16(trunk, shape, bc.trunk_grads(shape))
    assert trunk.pack_count == n_layers
    before = {k: host(p).copy() for k, p in trunk.named_parameters()}
    torch.optim.SGD(trunk.parameters(), lr=0.01).step()
    with torch.no_grad():
        maps = trunk(dev(tc.trunk_images(shape)))
    assert trunk.pack_count == 2 * n_layers                                # every trainable layer stepped: one launch each
    assert all(p.dtype == torch.float32 and (host(p) != before[k]).any() for k, p in trunk.named_parameters())
    fresh = DetectorTrunk.from_state_dict(trunk.state_dict(), dtype=BF16, device='cuda')      # an inference trunk from the stepped masters
    with torch.no_grad():
        for l, (got, want) in enumerate(zip(maps, fresh(dev(tc.trunk_images(shape))))):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f'map {l} after the step'
        trunk(dev(tc.trunk_images(shape)))
    assert trunk.pack_count == 2 * n_layers                                # a second forward packs nothing
    assert all(v.dtype == torch.float32 for v in trunk.state_dict().values() if v.is_floating_point())
    assert isinstance(trunk.stem, TrunkLayer) and trunk.stem.dtype == BF16 and not hasattr(trunk.stem, 'weight')      # frozen: packed once, in bfloat16


def test_a_training_step_of_the_whole_detector_on_a_bfloat16_trunk():
    from test_detector_trunk_backward import e2e_frames, e2e_targets
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()}
    det = Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=RESIZE, trainable=True, train_dtype=BF16)
    assert det.trainable and det.trunk.train_dtype == BF16
    head_layers = [l for l in det.heads.layers() if isinstance(l, TrainableLayer)]
    assert head_layers and all(l.dtype == torch.float32 and l.w.dtype == torch.float32 for l in head_layers)      # the unchanged float32 heads
    rng = np.random.RandomState(5)
    with torch.no_grad():
        n_anchors = 3 * sum(int(m.shape[2] * m.shape[3]) for m in det.trunk(torch.zeros(2, 3, 64, 64, device='cuda')))
    keys = dict(rpn=dev(rng.randint(0, 2 ** 31 - 1, (2, n_anchors)).astype(np.int32)), roi=dev(rng.randint(0, 2 ** 31 - 1, (2, 2000 + 2)).astype(np.int32)))

    def run():
        det.zero_grad()
        losses = det.losses(e2e_frames(), e2e_targets(), keys=keys)
        sum(losses.values()).backward()
        return losses, {k: p.grad.clone() for k, p in det.named_parameters()}
    losses, grads = run()
    assert set(losses) == {'loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg', 'loss_mask'}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert len(grads) == len(det.named_parameters())
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(bool(g.any()) for k, g in grads.items() if 'layer2.0.conv1' in k) and any(bool(g.any()) for k, g in grads.items() if 'fpn.inner_blocks.0' in k)
    assert any(bool(g.any()) for k, g in grads.items() if k.startswith('rpn.head.')) and any(bool(g.any()) for k, g in grads.items() if k.startswith('roi_heads.'))
    losses2, again = run()                                                   # a second run is bit-equal to the first
    assert all(torch.equal(grads[k].view(torch.int32), again[k].view(torch.int32)) for k in grads)
    assert all(torch.equal(losses[k].view(torch.int32), losses2[k].view(torch.int32)) for k in losses)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(call, start):
    rc = call()
    msg = _lib.lib().cosy_last_error().decode()
    assert rc != 0 and msg.startswith(start), (rc, msg)
    return msg


def test_the_bfloat16_entry_points_refuse_before_any_launch():
    L = _lib.lib()
    C, O, B, H, W = 8, 16, 1, 5, 7
    g = torch.zeros((B * H * W, O), dtype=BF16, device='cuda')
    w = torch.zeros(64 * 9 * 32, dtype=BF16, device='cuda')
    out = torch.zeros((B * H * W, C), dtype=BF16, device='cuda')
    add = torch.zeros((B * 12 * 16, C), dtype=BF16, device='cuda')

    def layer(**kw):
        d = _lib.HeadLayer()
        d.x, d.w, d.out = _lib.ptr(g), _lib.ptr(w), _lib.ptr(out)
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_BF16, 3, O, C, 0, _lib.HEAD_STORE_ROWS, C, 1
        d.row_start[0], d.row_start[1], d.H[0], d.W[0] = 0, B * H * W, H, W
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def dgrad(d, stride=1, add0=None, rule0=0, h0=0, w0=0, add1=None, rule1=0, h1=0, w1=0, y=None):
        return lambda: L.cosy_trunk_dgrad16(ctypes.byref(d), stride, add0, rule0, h0, w0, add1, rule1, h1, w1, y, None)
    a = _lib.ptr(add)
    for call in (dgrad(layer(), stride=3), dgrad(layer(ksize=1), stride=2), dgrad(layer(), rule0=7, add0=a), dgrad(layer(), add0=a, rule0=_lib.TRUNK_ADD_EVEN, h0=3, w0=3),
                 dgrad(layer(), add1=a, rule1=_lib.TRUNK_ADD_NEAREST_T, h1=4, w1=7), dgrad(layer(c_out=12)), dgrad(layer(c_in=20)), dgrad(layer(ksize=2)),
                 dgrad(layer(x=_lib.ptr(g) + 4)), dgrad(layer(), y=_lib.ptr(out) + 8), dgrad(layer(), add0=a + 4, rule0=_lib.TRUNK_ADD_SAME),
                 dgrad(layer(dtype=_lib.COSY_F16)), dgrad(layer(dtype=_lib.COSY_F32)), dgrad(layer(relu=1)), dgrad(layer(store=_lib.HEAD_STORE_DECONV_ROWS)),
                 dgrad(layer(store=_lib.HEAD_STORE_NCHW)), dgrad(layer(), add0=None, rule0=_lib.TRUNK_ADD_SAME)):
        refused(call, 'cosy_trunk_dgrad16:')
    assert 'loss scaler' in refused(dgrad(layer(dtype=_lib.COSY_F16)), 'cosy_trunk_dgrad16:')
    two = layer(n_levels=2)
    two.row_start[1], two.row_start[2], two.H[1], two.W[1] = B * H * W, B * H * W, H, W
    assert 'one level' in refused(dgrad(two, stride=2), 'cosy_trunk_dgrad16:')
    big = layer()
    big.H[0], big.W[0], big.row_start[1] = 1 << 14, 1 << 15, 3 << 29                # three maps of 2^29 cells
    assert '2^30' in refused(dgrad(big), 'cosy_trunk_dgrad16:')
    empty = layer()
    empty.row_start[1] = 0
    assert dgrad(empty)() == 0 and dgrad(empty, stride=2)() == 0            # M = 0 launches nothing

    x = torch.zeros((B * H * W, C), dtype=BF16, device='cuda')
    dw, db = torch.ones((O, C, 3, 3), device='cuda'), torch.ones(O, device='cuda')
    need = int(L.cosy_head_wgrad_workspace_bytes(B * 3 * 4, 3, C, O))
    ws = torch.zeros(need // 4, device='cuda')

    def wl(**kw):
        d = layer(c_in=C, c_out=O, n_split=O, x=_lib.ptr(x))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def wgrad(d, stride=2, nbytes=need, gp=None):
        return lambda: L.cosy_trunk_wgrad16(ctypes.byref(d), stride, _lib.ptr(g) if gp is None else gp, None, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, None)
    for call in (wgrad(wl(), stride=0), wgrad(wl(c_in=12)), wgrad(wl(c_out=20)), wgrad(wl(ksize=2)), wgrad(wl(dtype=_lib.COSY_F32)), wgrad(wl(dtype=_lib.COSY_F16)),
                 wgrad(wl(), gp=_lib.ptr(g) + 8), wgrad(wl(x=_lib.ptr(x) + 8))):
        refused(call, 'cosy_trunk_wgrad16:')
    assert 'workspace_bytes' in refused(wgrad(wl(), nbytes=need - 4), 'cosy_trunk_wgrad16:')
    two = wl(n_levels=2)
    two.row_start[1], two.row_start[2], two.H[1], two.W[1] = B * H * W, B * H * W, H, W
    assert 'one level' in refused(wgrad(two), 'cosy_trunk_wgrad16:')
    empty = wl()
    empty.row_start[1] = 0
    assert wgrad(empty)() == 0                                              # T = 0: zeros of the right shape
    torch.cuda.synchronize()
    assert not host(dw).any() and not host(db).any()

    def pack(**kw):                                                         # no call here gets as far as a launch: the three outputs may alias
        args = dict(w=_lib.ptr(dw), scale=None, shift=_lib.ptr(db), ksize=3, c_in=C, c_out=O, fwd=_lib.ptr(w), fwd_bias=_lib.ptr(ws), bwd=_lib.ptr(w), stream=None)
        args.update(kw)
        return lambda: L.cosy_trunk_weight_pack16(*args.values())
    for call in (pack(ksize=2), pack(c_in=12), pack(c_out=4), pack(w=None), pack(shift=None), pack(bwd=_lib.ptr(w) + 4)):
        refused(call, 'cosy_trunk_weight_pack16:')
    rows = torch.zeros((4, 8), dtype=BF16, device='cuda')
    for call in (lambda: L.cosy_trunk_grad_pack16(None, _lib.ptr(rows), 1, 12, 4, None), lambda: L.cosy_trunk_grad_pack16(None, _lib.ptr(rows), 1, 8, 0, None),
                 lambda: L.cosy_trunk_grad_pack16(None, None, 1, 8, 4, None), lambda: L.cosy_trunk_grad_pack16(None, _lib.ptr(rows) + 2, 1, 8, 4, None)):
        refused(call, 'cosy_trunk_grad_pack16:')
    assert L.cosy_trunk_grad_pack16(None, None, 0, 8, 4, None) == 0


def test_train_dtype_is_refused_where_it_cannot_apply():
    sd = bc.torch_sd()
    with pytest.raises(ValueError, match='loss scaler'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float16)
    with pytest.raises(ValueError, match='trainable=True'):
        DetectorTrunk.from_state_dict(sd, device='cuda', train_dtype=BF16)
    same = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float32)      # today's path under its own name
    assert same.train_dtype == torch.float32 and same.dtype == torch.float32 and all(l.w.dtype == torch.float32 for l in same.layers())
    trunk = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_dtype=BF16)
    images = dev(tc.trunk_images(tc.INPUTS[0]))
    with pytest.raises(RuntimeError, match='stem'):
        trunk(images.clone().requires_grad_())
    out = trunk(images)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(out[0].sum(), trunk.parameters()[0], create_graph=True)
    with torch.no_grad():                                                   # under no_grad the call IS the bfloat16 inference path
        plain = DetectorTrunk.from_state_dict(sd, dtype=BF16, device='cuda')
        assert all(torch.equal(a, b) for a, b in zip(trunk(images), plain(images)))
    assert trunk.last_kept_bytes == tb.kept_bytes(out[0].grad_fn.keep) > 0
    with pytest.raises(ValueError, match='float32 or bfloat16'):
        TrainableTrunkLayer('l', torch.zeros(8, 8, 1, 1), bias=torch.zeros(8), device='cuda', dtype=torch.float16)

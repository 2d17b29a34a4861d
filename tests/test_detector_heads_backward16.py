"""The backward of the detector's heads on bfloat16 rows on the GPU (csrc/kernels_detbwd16.hip behind cosypose_amd/detector_heads.py, DESIGN.md
section 32) against the CPU twin tests/detheadbwd16_ref.py, which test_detector_heads_backward16_host.py holds against torch.autograd in float64.

Criteria.  Every numeric check is ONE launch against float64 on that launch's own device operands (bf16-exact g, x, y and packed weight).
Packings: bytes.  Forward: bit-equal to the bfloat16 inference heads.  Data gradient: b = (K + 2) 2^-23 S with S = sum |ws g|, K = taps x the o
summed; an NCHW float32 store lies within b of t64, a row store within b + 2^-8 (|t64| + b), and is exactly +0.0 where the mask blocks.  Weight
gradient: (T + 2) 2^-23 S_W, bias gradient (T + 1) 2^-23 S_b, T the cells summed.  Two calls give equal bits.  Every test prints its largest
error as a share of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import dethead_case as fc
import dethead_ref as ref
import detheadbwd_case as bc
import detheadbwd16_ref as r16
from cosypose_amd import Detector, DetectorHeads, TrainableLayer, layer_backward
from cosypose_amd import _lib, detector_heads as dh

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def u16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def rows_of(a):
    """NCHW numpy -> bfloat16 device rows (B H W, C), rounded to nearest even; a linear layer's (M, K) is its own rows"""
    t = dev(a)
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.contiguous().to(BF16)


def nchw_of(rows, B, H, W):
    """device rows (B H W, C) -> float32 numpy (B, C, H, W)"""
    return host(rows).reshape(B, H, W, -1).transpose(0, 3, 1, 2)


def share_of(name, err, bound):
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest share of the bound = {share:.3f}')
    return share


def check_dgrad(name, got, d, rows):
    """got: float32 numpy in t64's shape; rows: the launch stored bfloat16 rows (mask and rounding), else float32 NCHW"""
    b, b16 = r16.dgrad_bound(d)
    bound = b16 if rows else b
    fin = np.isfinite(d['t64']) & ~d['blocked']
    err = np.abs(got.astype(np.float64) - d['t64'])
    share_of(name, err[fin], bound[fin])
    assert (err[fin] <= bound[fin]).all(), name
    assert np.array_equal(np.isnan(got[~d['blocked']]), np.isnan(d['t64'][~d['blocked']])), name
    assert not bits(got)[d['blocked']].any(), f'{name}: a blocked value is not +0.0'


def check_wgrad(name, dW, db, d):
    bW, bb = r16.wgrad_bound(d)
    for part, got, want, bound in (('dW', dW, d['dW'], bW), ('db', db, d['db'], bb)):
        got = np.asarray(got)
        assert got.shape == want.shape and got.dtype == F32, (name, part, got.shape, want.shape)
        err = np.abs(got.astype(np.float64) - want)
        share_of(f'{name} {part}', err, bound)
        assert (err <= bound).all(), (name, part)


def trainable_layer(layer, dtype=BF16):
    make = {'conv': TrainableLayer.conv, 'linear': TrainableLayer.linear, 'deconv': TrainableLayer.deconv}[layer['kind']]
    return make(torch.from_numpy(layer['weight']), torch.from_numpy(layer['bias']), relu=layer['relu'], device='cuda', dtype=dtype)


@pytest.fixture(scope='module')
def sd():
    return {k: torch.from_numpy(v) for k, v in fc.head_weights().items()}


def heads16(sd):
    return DetectorHeads.from_state_dict(sd, device='cuda', trainable=True, train_dtype=BF16)


# ---- packings --------------------------------------------------------------------------------------------------------------------------------
PACK_CASES = (('conv3', 40, 88, False, 1, 25, 41), ('conv1', 40, 15, False, 2, 5, 7), ('linear', 392, 15, False, 5, 1, 1), ('deconv', 16, 8, True, 3, 14, 14))


def test_the_device_pack_writes_the_bytes_of_the_bfloat16_host_packing(sd):
    heads = heads16(sd)
    plain = DetectorHeads.from_state_dict(sd, dtype=BF16, device='cuda')
    hw = fc.head_weights()
    twins = ref.rpn_layers(hw) + ref.box_layers(hw) + ref.mask_layers(hw)
    assert heads.dtype == torch.float32 and heads.train_dtype == BF16
    for i, (tl, pl, twin) in enumerate(zip(heads.layers(), plain.layers(), twins)):
        tl.refresh()
        assert tl.dtype == BF16 and tl.w.dtype == BF16 and tl.w_t.dtype == BF16 and all(p.dtype == torch.float32 for p in tl.parameters())
        assert np.array_equal(u16(tl.w), u16(pl.packed)), f'layer {i}: forward packing against the inference heads'
        assert np.array_equal(u16(tl.w), r16.pack_fwd16(twin)), f'layer {i}: forward packing against the twin'
        assert np.array_equal(bits(host(tl.bias)), bits(pl.packed_bias.numpy())), f'layer {i}: bias'
        assert np.array_equal(u16(tl.w_t), r16.pack_bwd16(twin)), f'layer {i}: transposed packing'
    for c in PACK_CASES:
        layer, _ = fc.case_data(c)
        tl = trainable_layer(layer).refresh()
        make = {'conv': dh.HeadLayer.conv, 'linear': dh.HeadLayer.linear, 'deconv': dh.HeadLayer.deconv}[layer['kind']]
        pl = make(torch.from_numpy(layer['weight']), torch.from_numpy(layer['bias']), dtype=BF16)
        assert np.array_equal(u16(tl.w), u16(pl.packed)) and np.array_equal(u16(tl.w), r16.pack_fwd16(layer)), c
        assert np.array_equal(bits(host(tl.bias)), bits(r16.bias_pad(layer))) and np.array_equal(u16(tl.w_t), r16.pack_bwd16(layer)), c


def test_the_gradient_pack_rounds_to_nearest_even_and_pads_with_zeros():
    rng = np.random.RandomState(3)
    g0, g1 = rng.normal(0, 1, (2, 3, 5, 7)).astype(F32), rng.normal(0, 1, (2, 12, 5, 7)).astype(F32)
    g0.reshape(-1)[:5] = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, np.inf], F32)                 # ties up and down, a signed zero
    for a, b, n0, n1 in ((g0, g1, 3, 12), (g0, None, 3, 12), (None, g1, 3, 12), (g1, None, 12, 0)):
        rows = torch.full((2 * 35, dh._pad8(n0 + n1)), 7.0, dtype=BF16, device='cuda')
        dh._grad_pack(None if a is None else dev(a), None if b is None else dev(b), rows, 2, n0, n1, 35)
        want = r16.grad_rows(np.zeros((2, n0, 35), F32) if a is None else a, (np.zeros((2, n1, 35), F32) if b is None else b) if n1 else None)
        assert np.array_equal(u16(rows), want.reshape(-1)), (n0, n1, a is None, b is None)


# ---- single layers ---------------------------------------------------------------------------------------------------------------------
LAYER_CASES = list(fc.PATHS) + [('linear', 392, co, co == 24, M, 1, 1) for co in (24, 15) for M in (0, 1, 5, 65, 257, 1025)] + list(fc.DECONV)
EDGE_CASES = [('linear', 40, 15, False, M, 1, 1) for M in (31, 32, 33, 255, 256, 257, 515)]      # one k-step; the slab's edges and three slabs
THIN_CASES = [('conv3', 8, 24, True, 2, 5, 1), ('conv3', 8, 24, True, 2, 1, 5)]                  # a map one cell wide, one cell high


def operands(c):
    layer, x = fc.case_data(c)
    return r16.layer16(layer), r16.bf16(x), r16.bf16(bc.case_grad(c))


@pytest.mark.parametrize('c', LAYER_CASES + EDGE_CASES + THIN_CASES, ids=bc.case_id)
def test_a_layers_gradients_meet_the_float64_bounds(c):
    layer, x, g = operands(c)
    tl = trainable_layer(fc.case_data(c)[0])
    dx, grads = layer_backward(tl, dev(x), dev(g))
    again_dx, again = layer_backward(tl, dev(x), dev(g))
    name = bc.case_id(c)
    assert dx.dtype == torch.float32 and dx.shape == x.shape and all(t.dtype == torch.float32 for t in grads)
    check_dgrad(f'{name} dX (NCHW float32)', host(dx), r16.dgrad64(layer, g), rows=False)
    check_wgrad(name, host(grads[0]), host(grads[1]), r16.wgrad64(layer, x, g))
    assert torch.equal(dx, again_dx) and all(torch.equal(a, b) for a, b in zip(grads, again))
    if x.shape[0] == 0:
        assert not host(grads[0]).any() and not host(grads[1]).any() and tuple(grads[0].shape) == layer['weight'].shape
    assert layer_backward(tl, dev(x), dev(g), need_dx=False)[0] is None


def test_the_slabs_sit_where_the_edge_cases_expect_them():
    assert [dh.wgrad_slab_rows(c[4]) for c in EDGE_CASES] == [bc.SLAB] * len(EDGE_CASES)


def launch_dgrad(tl, c, g, y, store):
    """one cosy_head_dgrad16 launch of case c on the bf16-exact numpy g (and mask y, input-shaped) -> float32 numpy in the input's shape"""
    kind, ci, co, relu, B, H, W = c
    up = 2 if kind == 'deconv' else 1
    tl.refresh()
    g_rows = torch.zeros((B * up * H * up * W, dh._pad8(co)), dtype=BF16, device='cuda')
    g_rows[:, :co] = rows_of(g)
    maps = [(B, up * H, up * W)]
    if store == _lib.HEAD_STORE_ROWS:
        out = dh._dgrad(tl, g_rows, maps, store, torch.empty((B * H * W, ci), dtype=BF16, device='cuda'), y=None if y is None else rows_of(y))
        return host(out) if kind == 'linear' else nchw_of(out, B, H, W)
    shape = (B, ci) if kind == 'linear' else (B, ci, H, W)
    return host(dh._dgrad(tl, g_rows, maps, store, torch.empty(shape, dtype=torch.float32, device='cuda')))


@pytest.mark.parametrize('c', [fc.PATHS[1], fc.PATHS[3], ('linear', 392, 15, False, 65, 1, 1), fc.DECONV[0], THIN_CASES[0]], ids=bc.case_id)
def test_a_row_store_masks_and_rounds_once_what_the_nchw_store_writes_unrounded(c):
    layer, x, g = operands(c)
    tl = trainable_layer(fc.case_data(c)[0])
    y = r16.bf16(np.where(np.abs(x) < 0.3, 0, x).astype(F32))              # the stored rows of a layer below: zeros, negatives and positives
    d_free, d_mask = r16.dgrad64(layer, g), r16.dgrad64(layer, g, y)
    nchw = launch_dgrad(tl, c, g, None, _lib.HEAD_STORE_NCHW)
    free = launch_dgrad(tl, c, g, None, _lib.HEAD_STORE_ROWS)
    masked = launch_dgrad(tl, c, g, y, _lib.HEAD_STORE_ROWS)
    name = bc.case_id(c)
    check_dgrad(f'{name} NCHW', nchw, d_free, rows=False)
    check_dgrad(f'{name} rows', free, d_free, rows=True)
    check_dgrad(f'{name} rows, masked', masked, d_mask, rows=True)
    assert d_mask['blocked'].any() and not d_mask['blocked'].all()
    b, _ = r16.dgrad_bound(d_free)                                             # the two stores of one accumulator: one rounding apart, inside b of t64 both
    assert np.array_equal(bits(r16.bf16(nchw)), bits(free)), f'{name}: the row store is not the NCHW store rounded once'
    assert np.array_equal(bits(masked)[~d_mask['blocked']], bits(free)[~d_mask['blocked']])


def test_a_nan_reaches_exactly_its_receptive_field_and_a_zero_y_blocks_it():
    c = ('conv3', 8, 24, True, 2, 5, 7)
    layer, x, g = operands(c)
    g = g.copy()
    g[1, 3, 2, 3] = np.nan
    tl = trainable_layer(fc.case_data(c)[0])
    d = r16.dgrad64(layer, g)
    got = launch_dgrad(tl, c, g, None, _lib.HEAD_STORE_NCHW)
    n = int(np.isnan(d['t64']).sum())
    print(f'NaN cells of dX: device {int(np.isnan(got).sum())}, twin {n} of {got.size}')
    assert n == 9 * 8 and np.array_equal(np.isnan(got), np.isnan(d['t64'])) and not np.isnan(got[0]).any()
    check_dgrad('beside the NaN', got, d, rows=False)
    y = np.ones(x.shape, F32)
    y[1, :, 2, 3] = 0                                                           # the centre of the field: blocked, NaN included
    masked = launch_dgrad(tl, c, g, y, _lib.HEAD_STORE_ROWS)
    assert not bits(masked[1, :, 2, 3]).any() and int(np.isnan(masked).sum()) == 8 * 8
    # one layer alone: y = 0 exactly, -0.0, a negative and a NaN under a row store with the mask
    tl = TrainableLayer.linear(torch.eye(8), torch.zeros(8), device='cuda', dtype=BF16).refresh()
    gl = dev(np.arange(1, 9, dtype=F32)[None]).to(BF16)
    yl = dev(np.array([[0.0, -0.0, -1.0, np.nan, 1e-30, 2.0, 0.0, 3.0]], F32)).to(BF16)
    out = host(dh._dgrad(tl, gl, [(1, 1, 1)], _lib.HEAD_STORE_ROWS, torch.empty((1, 8), dtype=BF16, device='cuda'), y=yl))
    assert np.array_equal(bits(out), bits(np.array([[0, 0, 0, 4, 5, 6, 0, 8]], F32)))


def level_wgrad(layer, xs, gs):
    """the weight gradient of one launch over several levels: the float64 sums and measures add over the levels, T too"""
    out = r16.wgrad64(layer, xs[0], gs[0])
    for x, g in zip(xs[1:], gs[1:]):
        out = bc.add(out, r16.wgrad64(layer, x, g))
    return out


def test_the_3x3_over_three_levels_whose_boundaries_fall_inside_a_k_step():
    rng = np.random.RandomState(11)
    layer, _ = fc.case_data(('conv3', 8, 24, True, 2, 5, 7))
    l16 = r16.layer16(layer)
    tl = trainable_layer(layer).refresh()
    xs = [r16.bf16(rng.normal(0, 1, (2, 8, H, W)).astype(F32)) for H, W in fc.RPN_GRID]
    gs = [r16.bf16(rng.normal(0, 1, (2, 24, H, W)).astype(F32)) for H, W in fc.RPN_GRID]
    maps = [(2, H, W) for H, W in fc.RPN_GRID]
    assert [2 * H * W for H, W in fc.RPN_GRID] == [70, 24, 4]                  # rows 70 and 94: inside the k-steps [64, 96)
    x_rows, g_rows = torch.cat([rows_of(x) for x in xs]), torch.cat([rows_of(g) for g in gs])
    dW, db = dh._wgrad(tl, x_rows, g_rows, maps)
    check_wgrad('three levels', host(dW), host(db), level_wgrad(l16, xs, gs))
    flat = dh._dgrad(tl, g_rows, maps, _lib.HEAD_STORE_NCHW, torch.empty(8 * 98, dtype=torch.float32, device='cuda'))
    rows = dh._dgrad(tl, g_rows, maps, _lib.HEAD_STORE_ROWS, torch.empty((98, 8), dtype=BF16, device='cuda'), y=x_rows)
    start = 0
    for l, ((B, H, W), x, g) in enumerate(zip(maps, xs, gs)):
        n = B * H * W
        check_dgrad(f'level {l} NCHW', host(flat[8 * start:8 * (start + n)]).reshape(B, 8, H, W), r16.dgrad64(l16, g), rows=False)
        check_dgrad(f'level {l} rows', nchw_of(rows[start:start + n], B, H, W), r16.dgrad64(l16, g, x), rows=True)
        start += n


def test_the_sibling_split_writes_each_layers_real_outputs():
    rng = np.random.RandomState(13)
    w0, b0, w1, b1 = (rng.normal(0, 1, s).astype(F32) for s in ((3, 40), (3,), (12, 40), (12,)))
    tl = TrainableLayer.siblings((torch.from_numpy(w0), torch.from_numpy(b0)), (torch.from_numpy(w1), torch.from_numpy(b1)), 'linear', device='cuda', dtype=BF16).refresh()
    assert tl.n_split == 3 and tl.n_grad == 15
    twin = dict(kind='linear', weight=np.concatenate([w0, w1]), bias=np.concatenate([b0, b1]), relu=False)
    assert np.array_equal(u16(tl.w), r16.pack_fwd16(twin)) and np.array_equal(u16(tl.w_t), r16.pack_bwd16(twin))
    x, g = r16.bf16(rng.normal(0, 1, (70, 40)).astype(F32)), r16.bf16(rng.normal(0, 1, (70, 15)).astype(F32))
    g_rows = torch.full((70, 16), np.nan, dtype=BF16, device='cuda')                # the pack writes the pad column
    dh._grad_pack(dev(g[:, :3]), dev(g[:, 3:]), g_rows, 70, 3, 12, 1)
    assert not u16(g_rows[:, 15]).any()
    got = dh._wgrad(tl, rows_of(x), g_rows, [(70, 1, 1)])
    assert [tuple(t.shape) for t in got] == [(3, 40), (3,), (12, 40), (12,)]
    first, second = bc.split(r16.wgrad64(twin, x, g), 3)
    check_wgrad('cls (3)', host(got[0]), host(got[1]), first)
    check_wgrad('box (12)', host(got[2]), host(got[3]), second)


# ---- whole heads -----------------------------------------------------------------------------------------------------------------------
def run_heads(heads, grads_np=None, keep=False):
    feats_np, roi_np, mroi_np = fc.head_inputs()
    g = bc.head_grads() if grads_np is None else grads_np
    heads.zero_grad()
    for h in (heads.rpn_head, heads.box_head, heads.mask_head):
        h.keep_rows = keep
    feats, roi, mroi = [dev(f).requires_grad_() for f in feats_np], dev(roi_np).requires_grad_(), dev(mroi_np).requires_grad_()
    obj, dlt = heads.rpn_head(feats)
    logits, boxes = heads.box_head(roi)
    masks = heads.mask_head(mroi)
    outs = obj + dlt + [logits, boxes, masks]
    gs = [dev(gl[:, :fc.A]) for gl in g['rpn']] + [dev(gl[:, fc.A:]) for gl in g['rpn']] + [dev(g['box'][:, :fc.K]), dev(g['box'][:, fc.K:]), dev(g['mask'])]
    torch.autograd.backward(outs, gs)
    return ([t.detach() for t in outs], dict(rpn=[f.grad for f in feats], box=roi.grad, mask=mroi.grad), {k: p.grad.clone() for k, p in heads.named_parameters()})


def forward_of(heads):
    feats, roi, mroi = fc.head_inputs()
    with torch.no_grad():
        obj, dlt = heads.rpn_head([dev(f) for f in feats])
        return obj + dlt + list(heads.box_head(dev(roi))) + [heads.mask_head(dev(mroi))]


def test_the_three_heads_every_launch_meets_its_bound(sd):
    heads = heads16(sd)
    outs, dx, dp = run_heads(heads, keep=True)
    for l, (a, b) in enumerate(zip(outs, forward_of(DetectorHeads.from_state_dict(sd, dtype=BF16, device='cuda')))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'forward output {l} against the bfloat16 inference heads'
    assert all(t.dtype == torch.float32 for t in list(dp.values()) + dx['rpn'] + [dx['box'], dx['mask']])
    hw = {k: v for k, v in fc.head_weights().items()}
    g_np = bc.head_grads()
    got = {k: host(v) for k, v in dp.items()}

    # the RPN: gradient pack, the sibling 1x1 (weight gradient over three levels, masked row store), the 3x3 (weight gradient, NCHW per level)
    k = heads.rpn_head.last_rows
    conv, pred = (r16.layer16(l) for l in ref.rpn_layers(hw))
    maps, starts = k['maps'], k['starts']
    assert k['x'].dtype == BF16 and k['hidden'].dtype == BF16 and k['g'].dtype == BF16 and k['gh'].dtype == BF16
    assert np.array_equal(u16(k['g']), np.concatenate([r16.grad_rows(g) for g in g_np['rpn']]).reshape(-1))
    per = lambda rows: [nchw_of(rows[starts[l]:starts[l + 1]], *maps[l]) for l in range(len(maps))]
    x, hidden, g, gh = per(k['x']), per(k['hidden']), [a[:, :5 * fc.A] for a in per(k['g'])], per(k['gh'])
    cls, box = bc.split(level_wgrad(pred, hidden, g), fc.A)
    check_wgrad('rpn.head.cls_logits', got['rpn.head.cls_logits.weight'], got['rpn.head.cls_logits.bias'], cls)
    check_wgrad('rpn.head.bbox_pred', got['rpn.head.bbox_pred.weight'], got['rpn.head.bbox_pred.bias'], box)
    check_wgrad('rpn.head.conv', got['rpn.head.conv.weight'], got['rpn.head.conv.bias'], level_wgrad(conv, x, gh))
    for l in range(len(maps)):
        check_dgrad(f'rpn gh level {l}', gh[l], r16.dgrad64(pred, g[l], hidden[l]), rows=True)
        check_dgrad(f'rpn dX level {l}', host(dx['rpn'][l]), r16.dgrad64(conv, gh[l]), rows=False)

    # the box head: three linear layers
    k = heads.box_head.last_rows
    fc6, fc7, pred = (r16.layer16(l) for l in ref.box_layers(hw))
    assert all(k[n].dtype == BF16 for n in ('x', 'h6', 'h7', 'g', 'g7', 'g6'))
    assert np.array_equal(u16(k['g']), r16.grad_rows(g_np['box'][:, :, None]).reshape(-1))
    x, h6, h7, g, g7, g6 = (host(k[n]) for n in ('x', 'h6', 'h7', 'g', 'g7', 'g6'))
    g = g[:, :5 * fc.K]
    cls, box = bc.split(r16.wgrad64(pred, h7, g), fc.K)
    p = 'roi_heads.box_'
    check_wgrad(p + 'predictor.cls_score', got[p + 'predictor.cls_score.weight'], got[p + 'predictor.cls_score.bias'], cls)
    check_wgrad(p + 'predictor.bbox_pred', got[p + 'predictor.bbox_pred.weight'], got[p + 'predictor.bbox_pred.bias'], box)
    check_wgrad(p + 'head.fc7', got[p + 'head.fc7.weight'], got[p + 'head.fc7.bias'], r16.wgrad64(fc7, h6, g7))
    check_wgrad(p + 'head.fc6', got[p + 'head.fc6.weight'], got[p + 'head.fc6.bias'], r16.wgrad64(fc6, x, g6))
    check_dgrad('box g7', g7, r16.dgrad64(pred, g, h7), rows=True)
    check_dgrad('box g6', g6, r16.dgrad64(fc7, g7, h6), rows=True)
    check_dgrad('box dX', host(dx['box']).reshape(len(x), -1), r16.dgrad64(fc6, g6), rows=False)

    # the mask head: the 1x1 logits on (2H, 2W), the deconvolution, four 3x3 convolutions
    k = heads.mask_head.last_rows
    layers = [r16.layer16(l) for l in ref.mask_layers(hw)]
    (D, H, W), = k['maps']
    assert k['up'].dtype == BF16 and k['g_up'].dtype == BF16 and all(t.dtype == BF16 for t in k['rows'] + k['g_convs'])
    assert np.array_equal(u16(k['g']), r16.grad_rows(g_np['mask']).reshape(-1))
    rows = [nchw_of(t, D, H, W) for t in k['rows']]
    up, g, g_up = nchw_of(k['up'], D, 2 * H, 2 * W), nchw_of(k['g'], D, 2 * H, 2 * W)[:, :fc.K], nchw_of(k['g_up'], D, 2 * H, 2 * W)
    g_convs = [nchw_of(t, D, H, W) for t in k['g_convs']]
    names = [f'roi_heads.mask_head.mask_fcn{i}' for i in range(1, 5)] + ['roi_heads.mask_predictor.conv5_mask', 'roi_heads.mask_predictor.mask_fcn_logits']
    pairs = [(rows[i], g_convs[i]) for i in range(4)] + [(rows[4], g_up), (up, g)]
    for name, layer, (xin, gin) in zip(names, layers, pairs):
        check_wgrad(name, got[name + '.weight'], got[name + '.bias'], r16.wgrad64(layer, xin, gin))
    check_dgrad('mask g_up', g_up, r16.dgrad64(layers[5], g, up), rows=True)
    check_dgrad('mask deconv dX', g_convs[3], r16.dgrad64(layers[4], g_up, rows[4]), rows=True)
    for i in (3, 2, 1):
        check_dgrad(f'mask conv {i + 1} dX', g_convs[i - 1], r16.dgrad64(layers[i], g_convs[i], rows[i]), rows=True)
    check_dgrad('mask dX', host(dx['mask']), r16.dgrad64(layers[0], g_convs[0]), rows=False)

    _, dx2, dp2 = run_heads(heads)                                              # a second call: equal bits
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dx['rpn'] + [dx['box'], dx['mask']], dx2['rpn'] + [dx2['box'], dx2['mask']]))
    assert all(torch.equal(dp[n].view(torch.int32), dp2[n].view(torch.int32)) for n in dp)


def test_an_sgd_step_moves_the_float32_masters_and_the_forward_is_the_bfloat16_inference_heads(sd):
    heads = heads16(sd)
    assert heads.pack_count == 0
    run_heads(heads)
    n_layers = len(heads.layers())
    assert heads.pack_count == n_layers
    run_heads(heads)                                                          # no step: no pack
    assert heads.pack_count == n_layers
    before = {k: host(p).copy() for k, p in heads.named_parameters()}
    torch.optim.SGD(heads.parameters(), lr=0.05).step()
    assert all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 and (host(p) != before[k]).any() for k, p in heads.named_parameters())
    outs = forward_of(heads)
    assert heads.pack_count == 2 * n_layers
    fresh = DetectorHeads.from_state_dict(heads.state_dict(), dtype=BF16, device='cuda')      # inference heads from the stepped masters
    for l, (a, b) in enumerate(zip(outs, forward_of(fresh))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'output {l} after the step'
    forward_of(heads)
    assert heads.pack_count == 2 * n_layers                                # a second forward packs nothing
    assert all(v.dtype == torch.float32 for v in heads.state_dict().values())
    out = heads.mask_head(dev(fc.head_inputs()[2]).requires_grad_())
    with pytest.raises(RuntimeError, match='mask_head: double backward'):
        torch.autograd.grad(out.sum(), heads.mask_head.parameters()[0], create_graph=True)


# ---- the whole detector --------------------------------------------------------------------------------------------------------------------
def test_a_training_step_of_the_fully_bfloat16_detector():
    import dettrunk_case as tc
    from test_detector_trunk_backward import e2e_frames, e2e_targets
    from test_detector_trunk_backward16 import RESIZE
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()}
    det = Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=RESIZE, trainable=True, train_dtype=BF16, heads_train_dtype=BF16)
    assert det.trainable and det.trunk.train_dtype == BF16 and det.heads.train_dtype == BF16
    assert all(l.dtype == BF16 and l.w.dtype == BF16 for l in det.heads.layers())
    rng = np.random.RandomState(5)
    with torch.no_grad():
        n_anchors = 3 * sum(int(m.shape[2] * m.shape[3]) for m in det.trunk(torch.zeros(2, 3, 64, 64, device='cuda')))
    keys = dict(rpn=dev(rng.randint(0, 2 ** 31 - 1, (2, n_anchors)).astype(np.int32)), roi=dev(rng.randint(0, 2 ** 31 - 1, (2, 2000 + 2)).astype(np.int32)))

    def run(d):
        d.zero_grad()
        losses = d.losses(e2e_frames(), e2e_targets(), keys=keys)
        sum(losses.values()).backward()
        return losses, {k: p.grad.clone() for k, p in d.named_parameters()}
    losses, grads = run(det)
    assert set(losses) == {'loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg', 'loss_mask'}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert len(grads) == len(det.named_parameters())
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(bool(g.any()) for k, g in grads.items() if 'layer2.0.conv1' in k) and any(bool(g.any()) for k, g in grads.items() if 'fpn.inner_blocks.0' in k)
    assert any(bool(g.any()) for k, g in grads.items() if k.startswith('rpn.head.')) and any(bool(g.any()) for k, g in grads.items() if k.startswith('roi_heads.'))
    losses2, again = run(det)                                                # a second run is bit-equal to the first
    assert all(torch.equal(grads[k].view(torch.int32), again[k].view(torch.int32)) for k in grads)
    assert all(torch.equal(losses[k].view(torch.int32), losses2[k].view(torch.int32)) for k in losses)
    # heads_train_dtype=None beside a bfloat16 trunk is the call without the keyword, bit for bit
    plain = Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=RESIZE, trainable=True, train_dtype=BF16)
    named = Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=RESIZE, trainable=True, train_dtype=BF16, heads_train_dtype=None)
    assert named.heads.train_dtype == torch.float32 and all(l.dtype == torch.float32 for l in named.heads.layers())
    (la, ga), (lb, gb) = run(plain), run(named)
    assert all(torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)) for k in ga) and all(torch.equal(la[k], lb[k]) for k in la)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(call, start):
    rc = call()
    msg = _lib.lib().cosy_last_error().decode()
    assert rc != 0 and msg.startswith(start), (rc, msg)
    return msg


def test_the_bfloat16_entry_points_refuse_by_name_before_any_launch():
    L = _lib.lib()
    tl = TrainableLayer.linear(torch.zeros(3, 8), torch.zeros(3), device='cuda', dtype=BF16).refresh()
    x, g = torch.zeros((5, 8), dtype=BF16, device='cuda'), torch.zeros((5, 8), dtype=BF16, device='cuda')
    out, ws = [torch.ones_like(p) for p in tl.parameters()], torch.empty(1024, device='cuda')
    dx = torch.empty((5, 8), dtype=BF16, device='cuda')

    def layer(**kw):
        d = _lib.HeadLayer()
        d.x, d.w, d.out = _lib.ptr(x), _lib.ptr(tl.w_t), _lib.ptr(dx)
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_BF16, 1, 8, 8, 0, _lib.HEAD_STORE_ROWS, 8, 1
        d.row_start[1], d.H[0], d.W[0] = 5, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    dgrad = lambda d, y=None: (lambda: L.cosy_head_dgrad16(ctypes.byref(d), y, None))
    wgrad = lambda d, nbytes=4096, gp=None: (lambda: L.cosy_head_wgrad16(ctypes.byref(d), _lib.ptr(g) if gp is None else gp, _lib.ptr(out[0]), _lib.ptr(out[1]), None, None,
                                                                         _lib.ptr(ws), nbytes, None))
    wl = lambda **kw: layer(**{**dict(c_out=3, n_split=3), **kw})
    assert dgrad(layer())() == 0 and wgrad(wl())() == 0, L.cosy_last_error()
    for d in (layer(dtype=_lib.COSY_F16), layer(dtype=_lib.COSY_F32), layer(c_in=12), layer(c_out=12), layer(ksize=5), layer(n_levels=0), layer(n_levels=9), layer(relu=1),
              layer(store=_lib.HEAD_STORE_DECONV_ROWS), layer(store=_lib.HEAD_STORE_NCHW, n_split=4), layer(x=_lib.ptr(x) + 8), layer(ksize=2)):
        refused(dgrad(d), 'cosy_head_dgrad16:')
    assert 'loss scaler' in refused(dgrad(layer(dtype=_lib.COSY_F16)), 'cosy_head_dgrad16:')
    assert 'no y' in refused(dgrad(layer(store=_lib.HEAD_STORE_NCHW), y=_lib.ptr(x)), 'cosy_head_dgrad16:')
    refused(dgrad(layer(), y=_lib.ptr(x) + 8), 'cosy_head_dgrad16:')
    big = layer()
    big.row_start[1] = (1 << 30) + 1
    assert '2^30' in refused(dgrad(big), 'cosy_head_dgrad16:')
    empty = layer()
    empty.row_start[1] = 0
    assert dgrad(empty)() == 0
    for d in (wl(dtype=_lib.COSY_F32), wl(dtype=_lib.COSY_F16), wl(c_in=4), wl(n_levels=9), wl(n_split=0), wl(ksize=2), wl(x=_lib.ptr(x) + 8)):
        refused(wgrad(d), 'cosy_head_wgrad16:')
    refused(wgrad(wl(), gp=_lib.ptr(g) + 8), 'cosy_head_wgrad16:')
    assert 'workspace_bytes' in refused(wgrad(wl(), nbytes=16), 'cosy_head_wgrad16:')      # refused by name, not truncated
    assert wgrad(wl(**{}), nbytes=4096)() == 0
    zero = wl()
    zero.row_start[1] = 0
    assert wgrad(zero)() == 0                                                # M = 0: no GEMM, zero gradients
    torch.cuda.synchronize()
    assert not host(out[0]).any() and not host(out[1]).any()
    rows = torch.zeros((4, 8), dtype=BF16, device='cuda')
    for call in (lambda: L.cosy_head_grad_pack16(None, None, _lib.ptr(rows), 4, 0, 0, 1, None), lambda: L.cosy_head_grad_pack16(None, None, _lib.ptr(rows), 4, 3, 5, 0, None),
                 lambda: L.cosy_head_grad_pack16(None, None, None, 4, 3, 5, 1, None), lambda: L.cosy_head_grad_pack16(None, None, _lib.ptr(rows) + 2, 4, 3, 5, 1, None)):
        refused(call, 'cosy_head_grad_pack16:')
    assert L.cosy_head_grad_pack16(None, None, None, 0, 3, 5, 1, None) == 0
    w, b = tl.pairs[0]

    def pack(**kw):                                                         # no call here gets as far as a launch
        args = dict(w0=_lib.ptr(w), b0=_lib.ptr(b), w1=None, b1=None, ksize=1, c_in=8, n0=3, n1=0, fwd=_lib.ptr(tl.w), fwd_bias=_lib.ptr(tl.bias), bwd=_lib.ptr(tl.w_t),
                    stream=None)
        args.update(kw)
        return lambda: L.cosy_head_weight_pack16(*args.values())
    for call in (pack(ksize=4), pack(c_in=12), pack(n0=0), pack(n1=2), pack(ksize=2), pack(w0=None), pack(bwd=_lib.ptr(tl.w_t) + 4)):
        refused(call, 'cosy_head_weight_pack16:')


def test_train_dtype_is_refused_where_it_cannot_apply(sd):
    with pytest.raises(ValueError, match='loss scaler'):
        DetectorHeads.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float16)
    with pytest.raises(ValueError, match='trainable=True'):
        DetectorHeads.from_state_dict(sd, device='cuda', train_dtype=BF16)
    with pytest.raises(ValueError, match='float32 only'):
        DetectorHeads.from_state_dict(sd, dtype=BF16, device='cuda', trainable=True, train_dtype=BF16)
    same = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float32)      # section 28 under its own name
    assert same.train_dtype == torch.float32 and all(l.dtype == torch.float32 and l.w.dtype == torch.float32 for l in same.layers())
    base = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    a, b = run_heads(same), run_heads(base)
    assert all(torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)) for k in a[2])
    heads = heads16(sd)
    with torch.no_grad():                                                   # under no_grad the call IS the bfloat16 inference path
        out = heads.box_head(dev(fc.head_inputs()[1]).requires_grad_())
    assert out[0].grad_fn is None and torch.equal(out[0], DetectorHeads.from_state_dict(sd, dtype=BF16, device='cuda').box_head(dev(fc.head_inputs()[1]))[0])
    with pytest.raises(ValueError, match='float32 or bfloat16'):
        TrainableLayer.linear(torch.zeros(3, 8), torch.zeros(3), device='cuda', dtype=torch.float16)

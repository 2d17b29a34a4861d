"""The backward of the detector's heads on the GPU (csrc/kernels_detbwd.hip behind cosypose_amd/detector_heads.py)
against the CPU twin tests/detheadbwd_ref.py, which test_detector_heads_backward_host.py holds against torch.autograd in float64.

Criteria.  Data gradient: BIT-equal to the twin's fmaf chain (the forward GEMM's order over the transposed, flipped weight).  Weight and bias
gradient: |dW - dW64| <= (T + 2) 2^-24 S_W, |db - db64| <= (T + 1) 2^-24 S_b with T the cells summed, S = sum |g x| resp. sum |g|: T float32
additions in any order, one rounding each, the products exact inside the fmaf -- section 26's (K + 2) u S with the cells as the reduction.  Two
calls give equal bits.  Nothing here compares against MIOpen's or rocBLAS's gradients.  Every test prints its largest error as a share of its bound."""
import numpy as np
import pytest
import torch

import dethead_case as fc
import dethead_ref as ref
import detheadbwd_case as bc
import detheadbwd_ref as bref
from cosypose_amd import DetectorHeads, TrainableLayer, conv_layer, layer_backward
from cosypose_amd import _lib, detector_heads as dh, detector_train as dt

pytestmark = pytest.mark.gpu
U = bref.U32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape, got.dtype)
    differ = int((bits(got) != bits(want)).sum())
    print(f'{name}: values whose bits differ from the twin\'s chain: {differ} of {got.size}')
    assert differ == 0, name


def within(name, got, d, which):
    """which: 'W' or 'b' of a wgrad64 dict"""
    want, S, T = d['d' + which], d['S_' + which], d['T_' + which]
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape)
    bound = (T + (2 if which == 'W' else 1)) * U * S
    err = np.abs(got.astype(np.float64) - want)
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest share of the bound (T = {T}) = {share:.3f}')
    assert (err <= bound).all(), name


def trainable_layer(layer):
    make = {'conv': TrainableLayer.conv, 'linear': TrainableLayer.linear, 'deconv': TrainableLayer.deconv}[layer['kind']]
    return make(torch.from_numpy(layer['weight']), torch.from_numpy(layer['bias']), relu=layer['relu'], device='cuda')


@pytest.fixture(scope='module')
def sd():
    return {k: torch.from_numpy(v) for k, v in fc.head_weights().items()}


def test_the_library_cuts_its_slabs_where_the_cases_expect_them():
    assert dh.wgrad_slab_rows(1) == bc.SLAB and all(dh.wgrad_slab_rows(c[4]) == bc.SLAB for c in bc.SLAB_CASES)
    assert dh.wgrad_slab_rows(16 * bc.SLAB) == bc.SLAB and dh.wgrad_slab_rows(16 * bc.SLAB + 1) == bc.SLAB + 4       # never more than 16 slabs
    need = _lib.lib().cosy_head_wgrad_workspace_bytes
    assert need(1024, 1, 12544, 1024) == 4 * (1024 * 12544 + 1024) * 4                                             # fc6 fits: four slabs
    assert need(5, 4, 8, 8) == 0 and need(5, 1, 0, 8) == 0


# ---- single layers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', bc.CASES, ids=bc.case_id)
def test_a_layers_gradients_meet_the_chains_bits_and_the_float64_bound(c):
    layer, x = fc.case_data(c)
    g, want = bc.case_grad(c), bc.want(c)
    tl = trainable_layer(layer)
    dx, grads = layer_backward(tl, dev(x), dev(g))
    again_dx, again = layer_backward(tl, dev(x), dev(g))
    name = bc.case_id(c)
    same_bits(f'{name} dX', host(dx), want['dx32'])
    within(f'{name} dW', host(grads[0]), want, 'W')
    within(f'{name} db', host(grads[1]), want, 'b')
    assert torch.equal(dx, again_dx) and all(torch.equal(a, b) for a, b in zip(grads, again))
    if x.shape[0] == 0:
        assert not host(grads[0]).any() and not host(grads[1]).any() and tuple(grads[0].shape) == layer['weight'].shape
    assert layer_backward(tl, dev(x), dev(g), need_dx=False)[0] is None


def test_the_device_weight_pack_writes_the_host_packings_bytes(sd):
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    plain = DetectorHeads.from_state_dict(sd, device='cuda')
    for tl in heads.layers():
        tl.refresh()
    for i, (tl, pl) in enumerate(zip(heads.layers(), plain.layers())):
        assert np.array_equal(bits(host(tl.w)), bits(pl.packed.numpy())), f'layer {i}: forward packing'
        assert np.array_equal(bits(host(tl.bias)), bits(pl.packed_bias.numpy())), f'layer {i}: bias'
        wt = torch.cat([dh.transposed_weight(tl.kind, w) for w, _ in tl.pairs], 2)
        assert np.array_equal(bits(host(tl.w_t)), bits(dh.pack_weight(wt, torch.float32).numpy())), f'layer {i}: transposed packing'
    for c in (('conv3', 40, 88, False, 1, 25, 41), ('conv1', 40, 15, False, 2, 5, 7), ('linear', 392, 15, False, 5, 1, 1), ('deconv', 16, 8, True, 3, 14, 14)):
        layer, _ = fc.case_data(c)
        tl = trainable_layer(layer).refresh()
        make = {'conv': dh.HeadLayer.conv, 'linear': dh.HeadLayer.linear, 'deconv': dh.HeadLayer.deconv}[layer['kind']]
        pl = make(torch.from_numpy(layer['weight']), torch.from_numpy(layer['bias']))
        assert np.array_equal(bits(host(tl.w)), bits(pl.packed.numpy())) and np.array_equal(bits(host(tl.bias)), bits(pl.packed_bias.numpy())), c
        wt = dh.pack_weight(dh.transposed_weight(tl.kind, torch.from_numpy(layer['weight'])), torch.float32)
        assert np.array_equal(bits(host(tl.w_t)), bits(wt.numpy())), c


# ---- whole heads -----------------------------------------------------------------------------------------------------------------------
def run_heads(heads, grads_np=None):
    """forward + backward of the three heads on dethead_case's inputs with detheadbwd_case's gradients -> outputs, input grads, param grads"""
    feats_np, roi_np, mroi_np = fc.head_inputs()
    g = bc.head_grads() if grads_np is None else grads_np
    heads.zero_grad()
    feats, roi, mroi = [dev(f).requires_grad_() for f in feats_np], dev(roi_np).requires_grad_(), dev(mroi_np).requires_grad_()
    obj, dlt = heads.rpn_head(feats)
    logits, boxes = heads.box_head(roi)
    masks = heads.mask_head(mroi)
    outs = obj + dlt + [logits, boxes, masks]
    gs = [dev(gl[:, :fc.A]) for gl in g['rpn']] + [dev(gl[:, fc.A:]) for gl in g['rpn']] + [dev(g['box'][:, :fc.K]), dev(g['box'][:, fc.K:]), dev(g['mask'])]
    torch.autograd.backward(outs, gs)
    return ([host(t) for t in outs], dict(rpn=[host(f.grad) for f in feats], box=host(roi.grad), mask=host(mroi.grad)),
            {k: host(p.grad) for k, p in heads.named_parameters()})


def test_the_three_heads_backward_equals_the_twins_chain(sd):
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    outs, dx, dp = run_heads(heads)
    fwd = fc.head_bits()
    for l, o in enumerate(fwd['rpn']):                                        # the float32 forward is the chain's: the masks are the twin's
        same_bits(f'rpn forward {l}', np.concatenate([outs[l], outs[3 + l]], 1), o)
    same_bits('box forward', np.concatenate(outs[6:8], 1), fwd['box'])
    same_bits('mask forward', outs[8], fwd['mask'])
    want = bc.head_wants()
    for l, w in enumerate(want['rpn'][0]):
        same_bits(f'rpn dX level {l}', dx['rpn'][l], w)
    same_bits('box dX', dx['box'], want['box'][0])
    same_bits('mask dX', dx['mask'], want['mask'][0])
    assert set(dp) == {f'{k}.{p}' for h in ('rpn', 'box', 'mask') for k in want[h][1] for p in ('weight', 'bias')}
    for h in ('rpn', 'box', 'mask'):
        for k, d in want[h][1].items():
            within(f'{k}.weight', dp[k + '.weight'], d, 'W')
            within(f'{k}.bias', dp[k + '.bias'], d, 'b')
    outs2, dx2, dp2 = run_heads(heads)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(dx['rpn'] + [dx['box'], dx['mask']], dx2['rpn'] + [dx2['box'], dx2['mask']]))
    assert all(np.array_equal(bits(dp[k]), bits(dp2[k])) for k in dp)


def test_no_grad_and_plain_inputs_take_the_inference_path_and_misuse_is_refused(sd):
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    plain = DetectorHeads.from_state_dict(sd, device='cuda')
    feats, roi, mroi = fc.head_inputs()
    with torch.no_grad():
        out = heads.box_head(dev(roi).requires_grad_())
        assert out[0].grad_fn is None and not out[0].requires_grad and torch.equal(out[0], plain.box_head(dev(roi))[0])
    out = heads.mask_head(dev(mroi))                                             # parameters require grad: a node, the same bits
    assert out.grad_fn is not None and torch.equal(out.detach(), plain.mask_head(dev(mroi)))
    for p in heads.parameters():
        p.requires_grad_(False)
    assert heads.mask_head(dev(mroi)).grad_fn is None
    assert heads.rpn_head([dev(f).requires_grad_(l == 1) for l, f in enumerate(feats)])[0][0].grad_fn is not None
    for p in heads.parameters():
        p.requires_grad_(True)
    x = dev(roi).requires_grad_()
    logits, _ = heads.box_head(x)
    with pytest.raises(RuntimeError, match='box_head: double backward'):
        torch.autograd.grad(logits.sum(), x, create_graph=True)
    with pytest.raises(ValueError, match='float32'):
        heads.box_head(dev(roi).half())
    empty = heads.box_head(torch.zeros((0, fc.BOX_C, 7, 7), device='cuda').requires_grad_())
    heads.zero_grad()
    (empty[0].sum() + empty[1].sum()).backward()
    assert all(p.grad is not None and p.grad.shape == p.shape and not bool(p.grad.any()) for p in heads.box_head.parameters())


def test_c_abi_backward_refusals():
    lib = _lib.lib()
    tl = TrainableLayer.linear(torch.zeros(3, 8), torch.zeros(3), device='cuda').refresh()
    x, g = torch.zeros((5, 8), device='cuda'), torch.zeros((5, 8), device='cuda')
    out, ws = [torch.empty_like(p) for p in tl.parameters()], torch.empty(1024, device='cuda')

    def layer(**kw):
        d = _lib.HeadLayer()
        d.x, d.w, d.out = x.data_ptr(), tl.w_t.data_ptr(), torch.empty((5, 8), device='cuda').data_ptr()
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_F32, 1, 8, 8, 0, _lib.HEAD_STORE_ROWS, 8, 1
        d.row_start[1], d.H[0], d.W[0] = 5, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    import ctypes
    dgrad = lambda d: lib.cosy_head_dgrad(ctypes.byref(d), None, _lib.stream())
    wgrad = lambda d, nbytes=4096: lib.cosy_head_wgrad(ctypes.byref(d), g.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None, None, ws.data_ptr(), nbytes, _lib.stream())
    assert dgrad(layer()) == 0 and wgrad(layer(c_out=3, n_split=3)) == 0, lib.cosy_last_error()
    for bad, word in ((dict(dtype=_lib.COSY_F16), 'dtype'), (dict(c_in=12), 'c_in'), (dict(ksize=5), 'ksize'), (dict(n_levels=0), 'n_levels'),
                      (dict(n_levels=9), 'n_levels'), (dict(relu=1), 'relu'), (dict(store=_lib.HEAD_STORE_DECONV_ROWS), 'store')):
        assert dgrad(layer(**bad)) == -1 and word in lib.cosy_last_error().decode(), bad
    for bad, word in ((dict(dtype=_lib.COSY_BF16), 'dtype'), (dict(c_in=4), 'c_in'), (dict(n_levels=9), 'n_levels'), (dict(n_split=0), 'n_split')):
        assert wgrad(layer(**{**dict(c_out=3, n_split=3), **bad})) == -1 and word in lib.cosy_last_error().decode(), bad
    assert wgrad(layer(c_out=3, n_split=3), nbytes=16) == -1 and 'workspace_bytes' in lib.cosy_last_error().decode()      # refused by name, not truncated
    big = layer()
    big.row_start[1] = (1 << 30) + 1
    assert dgrad(big) == -1 and '2^30' in lib.cosy_last_error().decode()
    assert lib.cosy_head_grad_pack(None, None, g.data_ptr(), 5, 0, 0, 1, _lib.stream()) == -1
    assert lib.cosy_head_weight_pack(tl.pairs[0][0].data_ptr(), tl.pairs[0][1].data_ptr(), None, None, 1, 12, 3, 0, tl.w.data_ptr(), tl.bias.data_ptr(),
                                     tl.w_t.data_ptr(), _lib.stream()) == -1 and 'c_in' in lib.cosy_last_error().decode()
    torch.cuda.synchronize()


# ---- the ReLU mask rule ----------------------------------------------------------------------------------------------------------------
def test_a_nan_gradient_reaches_exactly_its_receptive_field_and_a_zero_y_blocks_it(sd):
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    g = {k: ([a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in bc.head_grads().items()}
    g['rpn'][0][1, 0, 2, 3] = np.nan                                             # one objectness gradient of image 1, level 0, cell (2, 3)
    g['mask'][2, 1, 9, 16] = np.nan
    _, dx, _ = run_heads(heads, g)
    hw = fc.head_weights()
    feats, _, mroi = fc.head_inputs()
    want_rpn, _ = bref.head_backward(ref.rpn_layers(hw), feats[0], g['rpn'][0])
    want_mask, _ = bref.head_backward(ref.mask_layers(hw), mroi, g['mask'])
    for name, got, want in (('rpn level 0', dx['rpn'][0], want_rpn), ('mask', dx['mask'], want_mask)):
        n = int(np.isnan(want).sum())
        print(f'{name}: NaN cells of dX: device {int(np.isnan(got).sum())}, twin {n} of {want.size}')
        assert 0 < n < want.size and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    assert not np.isnan(dx['rpn'][0][0]).any() and not np.isnan(dx['mask'][:2]).any()      # the other images see nothing of it
    # a stored y of exactly 0 blocks the gradient, NaN included: the hidden rows of the RPN at that cell hold zeros (ReLU) and the twin masks them
    hidden = ref.layer32(ref.rpn_layers(hw)[0], feats[0])
    zero = hidden[1, :, 2, 3] == 0
    assert zero.any() and not zero.all()
    # one layer alone: y = 0 exactly, -0.0, a negative and a NaN under a row store with the mask
    tl = TrainableLayer.linear(torch.eye(8), torch.zeros(8), device='cuda').refresh()
    gl = dev(np.arange(1, 9, dtype=np.float32)[None])
    y = dev(np.array([[0.0, -0.0, -1.0, np.nan, 1e-30, 2.0, 0.0, 3.0]], np.float32))
    out = host(dh._dgrad(tl, gl, [(1, 1, 1)], _lib.HEAD_STORE_ROWS, torch.empty((1, 8), device='cuda'), y=y))
    assert np.array_equal(bits(out), bits(np.array([[0, 0, 0, 4, 5, 6, 0, 8]], np.float32)))


# ---- the optimiser round trip ------------------------------------------------------------------------------------------------------------
def test_an_sgd_step_repacks_on_the_device_and_nothing_else_does(sd):
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    assert heads.pack_count == 0
    run_heads(heads)
    n_layers = len(heads.layers())
    assert heads.pack_count == n_layers
    run_heads(heads)                                                          # no step: no pack
    assert heads.pack_count == n_layers
    opt = torch.optim.SGD(heads.parameters(), lr=0.05)
    opt.step()
    stepped = {k: host(p) for k, p in heads.named_parameters()}
    assert any((stepped[k] != fc.head_weights()[k]).any() for k in stepped)
    feats, roi, mroi = fc.head_inputs()
    with torch.no_grad():
        obj, dlt = heads.rpn_head([dev(f) for f in feats])
        logits, boxes = heads.box_head(dev(roi))
        masks = heads.mask_head(dev(mroi))
    assert heads.pack_count == 2 * n_layers
    for l, f in enumerate(feats):
        same_bits(f'rpn after the step {l}', np.concatenate([host(obj[l]), host(dlt[l])], 1), ref.chain32(ref.rpn_layers(stepped), f))
    same_bits('box after the step', np.concatenate([host(logits), host(boxes)], 1), ref.chain32(ref.box_layers(stepped), roi.reshape(len(roi), -1)))
    same_bits('mask after the step', host(masks), ref.chain32(ref.mask_layers(stepped), mroi))
    with torch.no_grad():
        heads.mask_head(dev(mroi))
    assert heads.pack_count == 2 * n_layers
    # Adam takes the parameters as they are; a checkpoint's head keys go in and out
    torch.optim.Adam(heads.parameters(), lr=1e-3).step()
    out = heads.state_dict()
    assert set(out) == {k for k in fc.head_weights() if not k.startswith('backbone.')}
    heads.load_state_dict({k: torch.from_numpy(v) for k, v in fc.head_weights().items()})
    assert all(np.array_equal(host(p), fc.head_weights()[k]) for k, p in heads.named_parameters())
    with torch.no_grad():
        again = heads.mask_head(dev(mroi))
    assert heads.pack_count > 2 * n_layers
    same_bits('mask after load_state_dict', host(again), fc.head_bits()['mask'])


# ---- wiring: detector_losses through the trainable heads -------------------------------------------------------------------------------
def losses_backward(heads, feats, call):
    """one training forward + backward with the raw outputs' and the RoI features' gradients retained -> grads, captured tensors"""
    heads.zero_grad()
    seen = {}

    def keep(name, t):
        if t.requires_grad:
            t.retain_grad()
        seen[name] = t
        return t

    def rpn(fs):
        o, d = heads.rpn_head(fs)
        return [keep(f'obj{l}', t) for l, t in enumerate(o)], [keep(f'dlt{l}', t) for l, t in enumerate(d)]

    def box(roi):
        seen['box_in'] = keep('box_roi', roi)
        a, b = heads.box_head(roi)
        return keep('logits', a), keep('boxes', b)

    def mask(roi):
        seen['mask_in'] = keep('mask_roi', roi)
        return keep('masks', heads.mask_head(roi))
    losses = call(feats, rpn, box, mask)
    sum(losses.values()).backward()
    return {k: p.grad.clone() for k, p in heads.named_parameters()}, [None if f.grad is None else f.grad.clone() for f in feats], seen


def replay(heads, seen, L):
    """the gradients captured at the raw outputs, fed through the three heads' backward by hand -> param grads, rpn dX per level, box dX, mask dX"""
    heads.zero_grad()
    feats = [seen[f'rpn_in{l}'].detach().requires_grad_() for l in range(L)]
    roi, mroi = seen['box_in'].detach().requires_grad_(), seen['mask_in'].detach().requires_grad_()
    obj, dlt = heads.rpn_head(feats)
    logits, boxes = heads.box_head(roi)
    masks = heads.mask_head(mroi)
    outs = obj + dlt + [logits, boxes, masks]
    gs = [seen[f'obj{l}'].grad for l in range(L)] + [seen[f'dlt{l}'].grad for l in range(L)] + [seen['logits'].grad, seen['boxes'].grad, seen['masks'].grad]
    assert all(a.shape == b.shape for a, b in zip(outs, gs) if b is not None)
    torch.autograd.backward([o for o, b in zip(outs, gs) if b is not None], [b for b in gs if b is not None])
    return {k: p.grad.clone() for k, p in heads.named_parameters()}, [f.grad for f in feats], roi.grad, mroi.grad


def check_wiring(heads, feats_np, call, n_roi_levels, grads_on_features=True):
    L = len(feats_np)
    runs = []
    for _ in range(2):
        feats = [dev(f).requires_grad_(grads_on_features) for f in feats_np]
        dp, df, seen = losses_backward(heads, feats, call)
        for l, f in enumerate(feats):
            seen[f'rpn_in{l}'] = f
        runs.append((dp, df, seen))
    dp, df, seen = runs[0]
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in dp.values()), [k for k, v in dp.items() if not bool(v.any())]
    if grads_on_features:
        assert all(f is not None and bool(torch.isfinite(f).all()) and bool(f.any()) for f in df)
    else:
        assert all(f is None for f in df) and seen['box_roi'].grad is None
    assert all(torch.equal(dp[k], runs[1][0][k]) for k in dp)                                      # two runs give equal bits
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(df, runs[1][1]))
    rp, rf, rroi, rmroi = replay(heads, seen, L)
    differ = [k for k in dp if not torch.equal(dp[k], rp[k])]
    print(f'parameter gradients whose bits differ from the replay: {differ} of {len(dp)}')
    assert not differ
    if grads_on_features:
        assert torch.equal(seen['box_roi'].grad, rroi) and torch.equal(seen['mask_roi'].grad, rmroi)
        for l in range(n_roi_levels, L):                                                           # no RoIAlign reads these levels: the RPN's dX alone
            assert torch.equal(df[l], rf[l]), l


def test_detector_losses_backward_fills_every_gradient_through_the_heads():
    import test_detector_train as tt
    feats, gt, labels, masks, keys = tt.chain_case()
    sd = {k: torch.from_numpy(v) for k, v in fc.chain_weights().items()}
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    call = lambda fs, rpn, box, mask: dt.detector_losses(fs, rpn, box, mask, tt.targets_of(gt, labels, masks), tt.NETS, tt.PAD, n_roi_levels=2,
                                                         keys={k: dev(v) for k, v in keys.items()}, sizes=tt.SIZES, aspect_ratios=tt.RATIOS, **tt.CHAIN_RPN)
    check_wiring(heads, feats, call, 2)
    # the heads themselves, not wrappers: the signature of detector_losses is unchanged
    heads.zero_grad()
    fs = [dev(f).requires_grad_() for f in feats]
    sum(call(fs, heads.rpn_head, heads.box_head, heads.mask_head).values()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in heads.parameters()) and all(f.grad is not None for f in fs)


def test_head_fine_tuning_behind_a_frozen_trunk():
    import dettrunk_case as tc
    import test_detector_train as tt
    from cosypose_amd import DetectorTrunk
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()}
    trunk = DetectorTrunk.from_state_dict(sd, device='cuda')
    heads = DetectorHeads.from_state_dict(sd, device='cuda', trainable=True)
    shape = tc.INPUTS[0]
    with torch.no_grad():
        feats = [host(f) for f in trunk(dev(tc.trunk_images(shape)))]
    assert len(feats) == 5 and all(f.shape[1] == heads.rpn_head.conv.c_in for f in feats)
    rng = np.random.RandomState(5)
    gt = [np.array([[4, 6, 40, 44], [30, 20, 60, 58]], np.float32), np.array([[10, 10, 50, 40]], np.float32)]
    labels = [[1, 2], [1]]
    masks = [(rng.uniform(0, 1, (len(g),) + shape[2:]) < 0.5).astype(np.uint8) for g in gt]
    n_anchors = 3 * sum(f.shape[2] * f.shape[3] for f in feats)
    keys = dict(rpn=rng.randint(0, 2 ** 31 - 1, (2, n_anchors)).astype(np.int32), roi=rng.randint(0, 2 ** 31 - 1, (2, 20 + 2)).astype(np.int32))
    nets = [tuple(shape[2:])] * 2
    targets = [dict(boxes=dev(g), labels=dev(np.asarray(l, np.int64)), masks=dev(m)) for g, l, m in zip(gt, labels, masks)]
    call = lambda fs, rpn, box, mask: dt.detector_losses(fs, rpn, box, mask, targets, nets, tuple(shape[2:]), n_roi_levels=4,
                                                         keys={k: dev(v) for k, v in keys.items()}, sizes=((8,), (16,), (32,), (64,), (128,)),
                                                         aspect_ratios=tt.RATIOS, **tt.CHAIN_RPN)
    check_wiring(heads, feats, call, 4, grads_on_features=False)

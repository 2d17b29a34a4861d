"""The backward of the detector's trunk on the GPU (csrc/kernels_detbwd.hip behind cosypose_amd/detector_trunk_backward.py, DESIGN.md
section 29) against the CPU twin tests/dettrunkbwd_ref.py, which test_detector_trunk_backward_host.py holds against torch.autograd in float64.

Criteria.  Data gradient, with its add operands and its mask: BIT-equal to the twin's fmaf chain.  Weight gradient against the twin's float64 sums
over its own float32 operands: |dW - dW64| <= (T + 3) 2^-24 |scale[o]| S_W with a scale (section 28's T + 2 and one rounding for the scale
product), (T + 2) 2^-24 S_W for the FPN's weights, (T + 1) 2^-24 S_b for its biases; T the output cells summed.  Two calls give equal bits.
Every test prints its largest error as a share of its bound."""
import numpy as np
import pytest
import torch

import dettrunk_case as tc
import dettrunk_ref as tref
import dettrunkbwd_case as bc
import dettrunkbwd_ref as ref
from cosypose_amd import Detector, DetectorTrunk, TrainableTrunkLayer, TrunkLayer, layer_dgrad, layer_wgrad
from cosypose_amd import _lib, detector_trunk_backward as tb

pytestmark = pytest.mark.gpu
RULES = {ref.SAME: _lib.TRUNK_ADD_SAME, ref.EVEN: _lib.TRUNK_ADD_EVEN, ref.NEAREST_T: _lib.TRUNK_ADD_NEAREST_T}
RESIZE = (48, 64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(name, got, want, quiet=False):
    """equal bits; a NaN on one side must be a NaN on the other (its payload is the hardware's)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    differ = int(((bits(got) != bits(want)) & ~nan).sum()) + int((np.isnan(got) != nan).sum())
    if not quiet:
        print(f'{name}: values whose bits differ from the twin\'s chain: {differ} of {got.size} ({int(nan.sum())} NaN)')
    assert differ == 0, name
    return differ


def within(name, got, wg, quiet=False):
    """got: [dW (, db)] from the device, wg: the twin's wgrad64 dict"""
    bw, bb = ref.wgrad_bound(wg)
    worst = 0.0
    for which, g, want, bound in (('dW', got[0], wg['dW'], bw),) + ((('db', got[1], wg['db'], bb),) if wg['db'] is not None else ()):
        g = host(g)
        assert g.shape == want.shape and g.dtype == np.float32, (name, which, g.shape, want.shape)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan), (name, which, 'the NaNs are not where the twin has them')
        err = np.where(nan, 0.0, np.abs(g.astype(np.float64) - np.where(nan, 0.0, want)))
        ok = err <= np.where(nan, 0.0, bound)
        share = float((err / np.maximum(np.where(nan, 1.0, bound), 1e-300)).max()) if err.size else 0.0
        worst = max(worst, share)
        if not quiet:
            print(f'{name} {which}: max |err| = {float(err.max()):.3e}, largest share of the bound (T = {wg["T"]}) = {share:.3f}')
        assert ok.all(), (name, which)
    assert (len(got) == 2) == (wg['db'] is not None), name
    return worst


def trainable(layer, name='layer'):
    """a twin layer dict as a TrainableTrunkLayer: a FrozenBatchNorm with variance 1 and mean 0 gives exactly the scale and the shift"""
    O = layer['weight'].shape[0]
    w = torch.from_numpy(layer['weight'])
    if layer['scale'] is None:
        return TrainableTrunkLayer(name, w, bias=torch.from_numpy(layer['bias']), stride=layer['stride'], relu=layer['relu'], device='cuda')
    bn = (torch.from_numpy(layer['scale']), torch.from_numpy(layer['bias']), torch.zeros(O), torch.ones(O))
    return TrainableTrunkLayer(name, w, bn=bn, stride=layer['stride'], relu=layer['relu'], device='cuda')


# ---- single layers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', bc.DGRAD, ids=bc.case_id)
def test_a_data_gradient_meets_the_chains_bits(c):
    layer, g, ops, y = bc.dgrad_data(c)
    H, W = c[5][1:]
    tl = trainable(layer)
    call = lambda: layer_dgrad(tl, dev(g), H, W, [(RULES[r], dev(m)) for r, m in ops], None if y is None else dev(y))
    got = call()
    same_bits(c[0], host(got), bc.dgrad_want(c))
    assert torch.equal(got, call())
    if y is not None:                                         # a stored y of exactly 0 (or -0.0) blocks its element: +0.0, whatever arrives
        blocked = host(got)[y == 0]
        assert blocked.size and not blocked.any() and not np.signbit(blocked).any()


@pytest.mark.parametrize('c', bc.EVEN_CASES, ids=bc.case_id)
def test_a_strided_1x1_enters_through_the_even_rule_and_a_negative_zero_survives(c):
    down, conv1, g3, g1 = bc.even_data(c)
    B, H, W = c[1]
    want_d, want = bc.even_want(c)
    d = layer_dgrad(trainable(down), dev(g3), *g3.shape[2:], stride=1)
    same_bits(c[0] + ' on the output grid', host(d), want_d)
    got = host(layer_dgrad(trainable(conv1), dev(g1), H, W, [(_lib.TRUNK_ADD_EVEN, d)]))
    same_bits(c[0], got, want)
    assert got[0, 0, 1, 1] == 0 and np.signbit(got[0, 0, 1, 1]) and np.signbit(want[0, 0, 1, 1])      # an odd cell: no +0.0 was added to it


@pytest.mark.parametrize('c', bc.WGRAD, ids=bc.case_id)
def test_a_weight_gradient_meets_the_float64_bound(c):
    layer, x, g = bc.wgrad_data(c)
    tl = trainable(layer)
    got = layer_wgrad(tl, dev(x), dev(g))
    within(c[0], got, bc.wgrad_want(c))
    again = layer_wgrad(tl, dev(x), dev(g))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert tuple(got[0].shape) == layer['weight'].shape
    if c[6] == 'negative':
        assert (layer['scale'] < 0).all()


def test_the_slabs_sit_where_the_cases_expect_them():
    slab = _lib.lib().cosy_head_wgrad_slab_rows
    assert [slab(t) for t in (255, 256, 257, 515)] == [bc.SLAB] * 4 and -(-515 // bc.SLAB) == 3


def test_the_device_weight_pack_writes_the_host_packings_bytes():
    sd = bc.torch_sd()
    trunk = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=1)
    plain = DetectorTrunk.from_state_dict(sd, device='cuda')
    net = tc.trunk_net()
    twins = [l for blocks in net['stages'] for blk in blocks for l in [blk['conv1'], blk['conv2'], blk['conv3']] + ([blk['down']] if blk['down'] else [])]
    twins += net['inner'] + net['outer']
    layers, plains = trunk.layers()[1:], plain.layers()[1:]
    assert len(layers) == len(twins) == len(plains) and trunk.pack_count == 0
    for tl, pl, tw in zip(layers, plains, twins):
        tl.refresh()
        assert np.array_equal(bits(host(tl.w)), bits(pl.packed.numpy())), f'{tl.name}: forward packing'
        assert np.array_equal(bits(host(tl.bias)), bits(pl.packed_bias.numpy())), f'{tl.name}: shift'
        assert np.array_equal(bits(host(tl.w_t)), bits(ref.pack_bwd(tw))), f'{tl.name}: backward packing of ws'
        assert np.array_equal(bits(pl.packed.numpy()), bits(ref.pack_fwd(tw))) and np.array_equal(bits(pl.packed_bias.numpy()), bits(ref.pack_bias(tw)))
    assert trunk.pack_count == len(layers)
    for c in (bc.DGRAD[0], bc.DGRAD[-1], bc.WGRAD[-1]):       # widths that are no multiple of 16 or 64
        layer = (bc.dgrad_data(c) if c[0].startswith('d-') else bc.wgrad_data(c))[0]
        tl = trainable(layer).refresh()
        assert np.array_equal(bits(host(tl.w)), bits(ref.pack_fwd(layer))) and np.array_equal(bits(host(tl.w_t)), bits(ref.pack_bwd(layer))), c[0]
        assert np.array_equal(bits(host(tl.bias)), bits(ref.pack_bias(layer))), c[0]


# (name, ksize, c_in, c_out, (maps, H, W)): 3x3 with a partial channel group and every border tap; a 1x1 over 515 = 2 SLAB + 3 cells (three slabs,
# the last partial) whose second four-tile channel group is partial; a 3x3 whose maps are all border.  c_out % 8 == 0: both sides take it
SHARED = [('3x3 40->24 on 2 maps of 5x7', 3, 40, 24, (2, 5, 7)), ('1x1 88->24 on 1x515', 1, 88, 24, (1, 1, 515)), ('3x3 8->24 on 2 maps of 1x2', 3, 8, 24, (2, 1, 2))]


@pytest.mark.parametrize('c', SHARED, ids=lambda c: c[0].replace(' ', '_'))
def test_the_heads_and_the_trunks_entry_points_are_one_function(c):
    """cosy_head_weight_pack / _wgrad / _dgrad and cosy_trunk_weight_pack / _wgrad / _dgrad (stride 1, no scale, no add operand) end in the same
    kernels of csrc/kernels_detbwd.hip: the same parameters, x and g give the same BITS on both sides."""
    from cosypose_amd import TrainableLayer, layer_backward
    name, k, C, O, (B, H, W) = c
    rng = np.random.RandomState(28 + C)
    w, b = torch.from_numpy(rng.randn(O, C, k, k).astype(np.float32)), torch.from_numpy(rng.randn(O).astype(np.float32))
    x, g = dev(rng.randn(B, C, H, W).astype(np.float32)), dev(rng.randn(B, O, H, W).astype(np.float32))
    head = TrainableLayer.conv(w, b, device='cuda')
    trunk = TrainableTrunkLayer('shared', w, bias=b, stride=1, device='cuda')
    dx, (dw, db) = layer_backward(head, x, g)
    tw = layer_wgrad(trunk, x, g)
    tx = layer_dgrad(trunk, g, H, W)
    assert len(tw) == 2
    for what, got, want in (('dW', tw[0], dw), ('db', tw[1], db), ('dX', tx, dx), ('w', trunk.w, head.w), ('bias', trunk.bias, head.bias), ('w_t', trunk.w_t, head.w_t)):
        same_bits(f'{name} {what}', host(got), host(want))


# ---- the whole trunk -----------------------------------------------------------------------------------------------------------------------
def nchw(entry):
    rows, B, h, w = entry
    return host(rows.view(B, h, w, -1).permute(0, 3, 1, 2).contiguous())


def run_trunk(trunk, shape, grads):
    trunk.zero_grad()
    trunk.keep_rows = True
    out = trunk(dev(tc.trunk_images(shape)))
    torch.autograd.backward(out, [dev(g) for g in grads])
    return out, {k: p.grad.clone() for k, p in trunk.named_parameters()}, {k: nchw(v) for k, v in trunk.last_rows.items()}


def check_against_twin(name, pgrads, rows, want, tfs, prefix='backbone.'):
    names = {k for k in want['params'] if bc.trained(k, tfs)}
    assert {k.rsplit('.', 1)[0] for k in pgrads} == {prefix + k for k in names}
    assert set(rows) == {k for k in want['rows'] if bc.trained(k, tfs)}
    differ = sum(same_bits(k, v, want['rows'][k], quiet=True) for k, v in rows.items())
    print(f'{name}: {len(rows)} gradient row buffers, values whose bits differ from the twin\'s: {differ}')
    worst = 0.0
    for k in sorted(names):
        got = [pgrads[f'{prefix}{k}.weight']] + ([pgrads[f'{prefix}{k}.bias']] if f'{prefix}{k}.bias' in pgrads else [])
        worst = max(worst, within(k, got, want['params'][k], quiet=True))
    print(f'{name}: {len(names)} layers\' parameter gradients, largest share of a bound = {worst:.3f}')


@pytest.mark.parametrize('shape', tc.INPUTS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('tfs', bc.TRAIN_FROM)
def test_the_trunks_backward_is_the_twins(shape, tfs):
    trunk = DetectorTrunk.from_state_dict(bc.torch_sd(), device='cuda', trainable=True, train_from_stage=tfs)
    grads = bc.trunk_grads(shape)
    out, pgrads, rows = run_trunk(trunk, shape, grads)
    for l, (o, w) in enumerate(zip(out, tc.trunk_bits(shape)[0])):
        same_bits(f'forward map {tc_level(l)}', host(o), w, quiet=True)
    check_against_twin(f'train_from_stage={tfs}', pgrads, rows, bc.trunk_want(shape), tfs)
    frozen = [k for k, _ in trunk.named_parameters() if any(f'layer{s}.' in k for s in range(1, tfs)) or 'body.conv1' in k or '.bn' in k or 'downsample.1' in k]
    assert not frozen
    _, again, rows2 = run_trunk(trunk, shape, grads)                      # two calls give equal bits
    assert all(torch.equal(pgrads[k], again[k]) for k in pgrads) and all(np.array_equal(bits(rows[k]), bits(rows2[k])) for k in rows)


def tc_level(l):
    return ('0', '1', '2', '3', 'pool')[l]


def test_a_nan_reaches_what_the_twin_says_it_reaches():
    shape, tfs = tc.INPUTS[1], 2
    trunk = DetectorTrunk.from_state_dict(bc.torch_sd(), device='cuda', trainable=True, train_from_stage=tfs)
    want = bc.trunk_want(shape, 1, True)
    _, pgrads, rows = run_trunk(trunk, shape, bc.trunk_grads(shape, True))
    check_against_twin('a NaN in the gradient of map 2', pgrads, rows, want, tfs)
    hit = sorted(k for k, v in pgrads.items() if bool(torch.isnan(v).any()))
    clean = sorted(k for k, v in pgrads.items() if not bool(torch.isnan(v).any()))
    print(f'parameters a NaN reached: {len(hit)}, untouched: {len(clean)}')
    # bottom-up: the finer levels 0 and 1 never see it; level 2's output block, both laterals from there on and every stage below level 3's do
    assert all(any(f'fpn.{n}' in k for k in clean) for n in ('layer_blocks.0', 'layer_blocks.1', 'layer_blocks.3', 'inner_blocks.0', 'inner_blocks.1'))
    assert all(any(n in k for k in hit) for n in ('fpn.layer_blocks.2', 'fpn.inner_blocks.2', 'fpn.inner_blocks.3', 'layer4.', 'layer3.', 'layer2.'))
    assert not np.isnan(rows['fpn.G_inner.0']).any() and not np.isnan(rows['fpn.G_inner.1']).any()
    assert np.isnan(rows['fpn.G_inner.2']).any() and np.isnan(rows['fpn.G_inner.3']).any()


def test_two_forwards_before_one_backward_are_independent():
    trunk = DetectorTrunk.from_state_dict(bc.torch_sd(), device='cuda', trainable=True)
    a, b = tc.INPUTS
    out_a = trunk(dev(tc.trunk_images(a)))
    out_b = trunk(dev(tc.trunk_images(b)))                                # reuses the arena of the frozen stages; the kept rows are the node's own
    trunk.keep_rows = True
    torch.autograd.backward(out_a, [dev(g) for g in bc.trunk_grads(a)])
    rows = {k: nchw(v) for k, v in trunk.last_rows.items()}
    want = bc.trunk_want(a)
    assert sum(same_bits(k, v, want['rows'][k], quiet=True) for k, v in rows.items()) == 0
    del out_b


# ---- the optimiser round trip ------------------------------------------------------------------------------------------------------------
def test_an_sgd_step_repacks_the_stepped_layers_and_nothing_else_does():
    shape = tc.INPUTS[0]
    trunk = DetectorTrunk.from_state_dict(bc.torch_sd(), device='cuda', trainable=True)
    n_layers = sum(hasattr(l, 'weight') for l in trunk.layers())
    assert trunk.pack_count == 0
    run_trunk(trunk, shape, bc.trunk_grads(shape))
    assert trunk.pack_count == n_layers
    torch.optim.SGD(trunk.parameters(), lr=0.01).step()
    with torch.no_grad():
        maps = trunk(dev(tc.trunk_images(shape)))
    assert trunk.pack_count == 2 * n_layers                                # every trainable layer stepped: one launch each
    stepped = dict(tc.trunk_weights())
    changed = 0
    for k, p in trunk.named_parameters():
        changed += int((host(p) != stepped[k]).any())
        stepped[k] = host(p)
    assert changed == len(trunk.parameters())
    for l, (got, want) in enumerate(zip(maps, tref.trunk32(tref.net_from_sd(stepped), tc.trunk_images(shape)))):
        same_bits(f'map {tc_level(l)} after the step', host(got), want)
    with torch.no_grad():
        trunk(dev(tc.trunk_images(shape)))
    assert trunk.pack_count == 2 * n_layers                                # a second forward packs nothing
    sd = trunk.state_dict()
    assert set(sd) == {k for k in tc.trunk_weights() if k.startswith('backbone.')}
    fresh = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fresh(dev(tc.trunk_images(shape))), maps))
    fresh.load_state_dict(bc.torch_sd())
    with torch.no_grad():
        for l, (got, want) in enumerate(zip(fresh(dev(tc.trunk_images(shape))), tc.trunk_bits(shape)[0])):
            same_bits(f'map {tc_level(l)} after load_state_dict', host(got), want, quiet=True)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def e2e_frames():
    rng = np.random.RandomState(31)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for h, w in tc.E2E_FRAMES]


def e2e_targets():
    rng = np.random.RandomState(41)
    out = []
    for h, w in tc.E2E_FRAMES:
        boxes = np.array([[3, 4, w - 12, h - 9], [w // 3, h // 4, w - 4, h - 3]], np.float32)
        masks = np.zeros((2, h, w), np.uint8)
        for m, (x1, y1, x2, y2) in zip(masks, boxes.astype(int)):
            m[y1:y2, x1:x2] = rng.uniform(0, 1, (y2 - y1, x2 - x1)) < 0.8
        out.append(dict(boxes=dev(boxes), labels=dev(np.array([1, 2], np.int64)), masks=dev(masks)))
    return out


def e2e_run(det, keys):
    """one training forward + backward with the gradients at the trunk's five maps retained"""
    det.zero_grad()
    seen = {}
    trunk = det.trunk
    real = trunk.__class__.__call__

    class Spy:
        trainable = True

        def __call__(self, images):
            seen['images'] = images
            seen['maps'] = real(trunk, images)
            for m in seen['maps']:
                m.retain_grad()
            return seen['maps']
    trunk.keep_rows = True
    det.trunk = Spy()
    try:
        losses = det.losses(e2e_frames(), e2e_targets(), keys=keys)
    finally:
        det.trunk = trunk
    sum(losses.values()).backward()
    return losses, {k: p.grad.clone() for k, p in det.named_parameters()}, seen, {k: nchw(v) for k, v in trunk.last_rows.items()}


def test_a_training_step_of_the_whole_detector():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()}
    det = Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=RESIZE, trainable=True)
    assert det.train() is det and det.eval() is det
    rng = np.random.RandomState(5)
    with torch.no_grad():
        n_anchors = 3 * sum(int(m.shape[2] * m.shape[3]) for m in det.trunk(torch.zeros(2, 3, 64, 64, device='cuda')))
    keys = dict(rpn=dev(rng.randint(0, 2 ** 31 - 1, (2, n_anchors)).astype(np.int32)), roi=dev(rng.randint(0, 2 ** 31 - 1, (2, 2000 + 2)).astype(np.int32)))
    losses, grads, seen, rows = e2e_run(det, keys)
    assert set(losses) == {'loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg', 'loss_mask'}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert tuple(seen['images'].shape) == (2, 3, 64, 64)
    names = [k for k, _ in det.named_parameters()]
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and len(grads) == len(names)
    assert any(bool(g.any()) for k, g in grads.items() if 'layer2.0.conv1' in k) and any(bool(g.any()) for k, g in grads.items() if 'fpn.inner_blocks.0' in k)
    assert not [k for k in names if 'body.conv1' in k or 'layer1.' in k or '.bn' in k or 'downsample.1' in k or 'running' in k]      # the frozen ones hold none
    # the trunk's share: a replay of the captured gradients at the five maps through the twin
    # (the gradient retained at map '3' already holds the pool level's share, which autograd's slice backward added: pool's own is not replayed)
    map_grads = [None if m.grad is None else host(m.grad) for m in seen['maps'][:4]]
    assert seen['maps'][4].grad is not None and all(g is not None for g in map_grads)
    want = ref.trunk_backward(tc.trunk_net(), host(seen['images']), map_grads, 2)
    check_against_twin('the detector\'s losses', {k: g for k, g in grads.items() if k.startswith('backbone.')}, rows, want, 2)
    _, again, _, rows2 = e2e_run(det, keys)                                # a second run is bit-equal to the first
    assert all(torch.equal(grads[k], again[k]) for k in grads) and all(np.array_equal(bits(rows[k]), bits(rows2[k])) for k in rows)
    first = det.get_detections(e2e_frames(), output_masks=False)
    fresh = Detector.from_state_dict(det.state_dict(), tc.E2E_LABELS, input_resize=RESIZE, trainable=True)
    second = fresh.get_detections(e2e_frames(), output_masks=False)
    assert len(first) == len(second) > 0 and torch.equal(first.bboxes.view(torch.int32), second.bboxes.view(torch.int32))
    assert first.infos['label'].tolist() == second.infos['label'].tolist()
    assert np.array_equal(first.infos['score'].values.astype(np.float32).view(np.int32), second.infos['score'].values.astype(np.float32).view(np.int32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(call, start):
    rc = call()
    msg = _lib.lib().cosy_last_error().decode()
    assert rc != 0 and msg.startswith(start), (rc, msg)
    return msg


def test_the_entry_points_refuse_before_any_launch():
    import ctypes
    L = _lib.lib()
    C, O, B, H, W = 8, 16, 1, 5, 7
    g = torch.zeros((B * H * W, O), device='cuda')
    w = torch.zeros(64 * 9 * 16, device='cuda')
    out = torch.zeros((B * H * W, C), device='cuda')
    add = torch.zeros((B * 12 * 16, C), device='cuda')

    def layer(**kw):
        d = _lib.HeadLayer()
        d.x, d.w, d.out = _lib.ptr(g), _lib.ptr(w), _lib.ptr(out)
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_F32, 3, O, C, 0, _lib.HEAD_STORE_ROWS, C, 1
        d.row_start[0], d.row_start[1], d.H[0], d.W[0] = 0, B * H * W, H, W
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def dgrad(d, stride=1, add0=None, rule0=0, h0=0, w0=0, add1=None, rule1=0, h1=0, w1=0, y=None):
        return lambda: L.cosy_trunk_dgrad(ctypes.byref(d), stride, add0, rule0, h0, w0, add1, rule1, h1, w1, y, None)
    a = _lib.ptr(add)
    for call in (dgrad(layer(), stride=3), dgrad(layer(ksize=1), stride=2), dgrad(layer(), rule0=7, add0=a), dgrad(layer(), add0=a, rule0=_lib.TRUNK_ADD_EVEN, h0=3, w0=3),
                 dgrad(layer(), add1=a, rule1=_lib.TRUNK_ADD_NEAREST_T, h1=4, w1=7), dgrad(layer(c_out=12)), dgrad(layer(c_in=20)), dgrad(layer(ksize=2)),
                 dgrad(layer(x=_lib.ptr(g) + 4)), dgrad(layer(), y=_lib.ptr(out) + 8), dgrad(layer(), add0=a + 4, rule0=_lib.TRUNK_ADD_SAME),
                 dgrad(layer(dtype=_lib.COSY_F16)), dgrad(layer(relu=1)), dgrad(layer(store=_lib.HEAD_STORE_DECONV_ROWS))):
        refused(call, 'cosy_trunk_dgrad:')
    two = layer(n_levels=2)
    two.row_start[1], two.row_start[2], two.H[1], two.W[1] = B * H * W, B * H * W, H, W
    assert 'one level' in refused(dgrad(two, stride=2), 'cosy_trunk_dgrad:')
    big = layer()
    big.H[0], big.W[0], big.row_start[1] = 1 << 14, 1 << 15, 3 << 29                # three maps of 2^29 cells
    assert '2^30' in refused(dgrad(big), 'cosy_trunk_dgrad:')
    empty = layer()
    empty.row_start[1] = 0
    assert dgrad(empty)() == 0 and dgrad(empty, stride=2)() == 0            # M = 0 launches nothing

    x = torch.zeros((B * H * W, C), device='cuda')
    dw, db = torch.ones((O, C, 3, 3), device='cuda'), torch.ones(O, device='cuda')
    need = int(L.cosy_head_wgrad_workspace_bytes(B * 3 * 4, 3, C, O))
    ws = torch.zeros(need // 4, device='cuda')

    def wl(**kw):
        d = layer(c_in=C, c_out=O, n_split=O, x=_lib.ptr(x))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def wgrad(d, stride=2, nbytes=need):
        return lambda: L.cosy_trunk_wgrad(ctypes.byref(d), stride, _lib.ptr(g), None, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, None)
    for call in (wgrad(wl(), stride=0), wgrad(wl(c_in=12)), wgrad(wl(c_out=20)), wgrad(wl(ksize=2)), wgrad(wl(dtype=_lib.COSY_BF16))):
        refused(call, 'cosy_trunk_wgrad:')
    assert 'workspace_bytes' in refused(wgrad(wl(), nbytes=need - 4), 'cosy_trunk_wgrad:')
    two = wl(n_levels=2)
    two.row_start[1], two.row_start[2], two.H[1], two.W[1] = B * H * W, B * H * W, H, W
    assert 'one level' in refused(wgrad(two), 'cosy_trunk_wgrad:')
    empty = wl()
    empty.row_start[1] = 0
    assert wgrad(empty)() == 0                                              # T = 0: zeros of the right shape
    torch.cuda.synchronize()
    assert not host(dw).any() and not host(db).any()
    def pack(**kw):                                                         # no call here gets as far as a launch: the three outputs may alias
        args = dict(w=_lib.ptr(dw), scale=None, shift=_lib.ptr(db), ksize=3, c_in=C, c_out=O, fwd=_lib.ptr(w), fwd_bias=_lib.ptr(w), bwd=_lib.ptr(w), stream=None)
        args.update(kw)
        return lambda: L.cosy_trunk_weight_pack(*args.values())
    for call in (pack(ksize=2), pack(c_in=12), pack(c_out=4), pack(w=None), pack(shift=None), pack(bwd=_lib.ptr(w) + 4)):
        refused(call, 'cosy_trunk_weight_pack:')


def test_the_trainable_trunk_refuses_what_it_cannot_do():
    sd = bc.torch_sd()
    with pytest.raises(ValueError, match='float32 only'):
        DetectorTrunk.from_state_dict(sd, dtype=torch.float16, device='cuda', trainable=True)
    with pytest.raises(ValueError, match='stem'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=0)
    trunk = DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True)
    images = dev(tc.trunk_images(tc.INPUTS[0]))
    with pytest.raises(RuntimeError, match='stem'):
        trunk(images.clone().requires_grad_())
    out = trunk(images)
    (gw,) = torch.autograd.grad([o.sum() for o in out[:4]], [trunk.parameters()[0]], grad_outputs=[torch.ones((), device='cuda')] * 4, create_graph=False)
    assert bool(torch.isfinite(gw).all())
    out = trunk(images)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(out[0].sum(), trunk.parameters()[0], create_graph=True)
    with torch.no_grad():                                                   # under no_grad the call IS the inference path
        plain = DetectorTrunk.from_state_dict(sd, device='cuda')
        assert all(torch.equal(a, b) for a, b in zip(trunk(images), plain(images)))
    bad = dict(sd)
    bad['backbone.body.bn1.weight'] = sd['backbone.body.bn1.weight'] + 1
    with pytest.raises(ValueError, match='frozen'):
        trunk.load_state_dict(bad)
    with pytest.raises(KeyError, match='fpn.inner_blocks.0.bias'):
        trunk.load_state_dict({k: v for k, v in sd.items() if k != 'backbone.fpn.inner_blocks.0.bias'})
    assert isinstance(trunk.stem, TrunkLayer) and not hasattr(trunk.stem, 'weight')                      # the stem stays a packed constant
    assert trunk.last_kept_bytes == tb.kept_bytes(out[0].grad_fn.keep) > 0

"""The twin of the trunk's bfloat16 backward (tests/dettrunkbwd16_ref.py): its rounding against torch's, its packing
index rules against a dense loop, its float64 launch evaluations against torch.autograd in float64 on layers of dettrunk_case's narrow net fed
bf16-exact tensors, its bounds on a float32-accumulate emulation, and what train_dtype= refuses before it touches a device.  CPU only;
tests/test_detector_trunk_backward16.py holds the kernels against the twin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dettrunk_case as tc
import dettrunkbwd_case as bc
import dettrunkbwd16_ref as r16

F32 = np.float32


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def exact(rng, shape, spread=1.0):
    return r16.bf16(rng.normal(0, spread, shape).astype(F32))


# ---- rounding ----------------------------------------------------------------------------------------------------------------------------
def test_the_twins_rounding_is_torchs():
    rng = np.random.RandomState(16)
    one = np.float32(1.0).view(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,
                        0x00800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, one | 0x8000, one | 0x18000, one | 0x8001, one | 0x7FFF, one | 0x17FFF], np.uint32)
    a = np.concatenate([special, rng.randint(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32)]).view(F32)
    want = torch.from_numpy(a.copy()).to(torch.bfloat16)
    got = r16.bf16_bits(a)
    nan = np.isnan(a)
    assert np.array_equal(got[~nan], want.view(torch.int16).numpy().view(np.uint16)[~nan])
    assert np.isnan(r16.from_bits(got)[nan]).all() and torch.isnan(want.float()).numpy()[nan].all()         # a NaN stays a NaN (its payload is free)
    assert np.array_equal(np.signbit(r16.from_bits(got)[nan]), np.signbit(a[nan]))
    v = r16.bf16(a[~nan])
    assert r16.is_bf16(v) and np.array_equal(v.view(np.uint32), want.float().numpy()[~nan].view(np.uint32))
    assert r16.bf16_bits(np.array([1.0 + 2.0 ** -8], F32))[0] == 0x3F80 and r16.bf16_bits(np.array([1.0 + 3 * 2.0 ** -8], F32))[0] == 0x3F82      # ties to even
    assert r16.bf16_bits(np.array([-0.0], F32))[0] == 0x8000 and r16.bf16_bits(np.array([np.inf], F32))[0] == 0x7F80
    assert r16.bf16_bits(np.array([3.4028235e38], F32))[0] == 0x7F80                                         # the largest float32 rounds to inf


# ---- packings ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,ci,co,scaled', [(3, 8, 24, True), (1, 40, 72, False), (3, 72, 40, True), (1, 24, 8, True)])
def test_the_packing_rules_are_the_dense_loops(k, ci, co, scaled):
    rng = np.random.RandomState(ci + co + k)
    w = rng.normal(0, 1, (co, ci, k, k)).astype(F32)
    scale = -rng.uniform(0.5, 1.5, co).astype(F32) if scaled else None
    ws = r16.ws16(w, scale)
    if scaled:
        assert np.array_equal(ws, r16.bf16((w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(F32)))      # one product, one rounding
    else:
        assert np.array_equal(ws, r16.bf16(w))
    for name, op, packed in (('fwd', r16.fwd_operand(w), r16.pack_fwd16(w)), ('bwd', r16.bwd_operand(w, scale), r16.pack_bwd16(w, scale))):
        N, T, K = op.shape
        assert packed.dtype == np.uint16 and packed.size == (-(-N // 64) * 64) * T * (-(-K // 32) * 32), name
        dense = np.array([r16.pack16_at(op, i) for i in range(packed.size)], F32)
        assert np.array_equal(r16.from_bits(packed).view(np.uint32), dense.view(np.uint32)), name
    # fwd[n][tap][c] = bf16(w[n][c][tap]); bwd[c][tap][o] = ws[o][c][taps - 1 - tap]: transposed, the taps flipped
    fo, bo = r16.fwd_operand(w), r16.bwd_operand(w, scale)
    assert fo[3, k * k - 1, 5] == r16.bf16(w)[3, 5, k - 1, k - 1] and bo[5, 0, 3] == ws[3, 5, k - 1, k - 1] and bo[2, k * k - 1, 7] == ws[7, 2, 0, 0]
    # the host packing of the weight rounded to bfloat16 (what an inference trunk at dtype=torch.bfloat16 holds) has the same bytes
    from cosypose_amd.detector_heads import pack_weight
    host = pack_weight(torch.from_numpy(w).permute(0, 2, 3, 1).reshape(co, k * k, ci), torch.bfloat16)
    assert np.array_equal(host.view(torch.int16).numpy().view(np.uint16), r16.pack_fwd16(w))


# ---- one launch against autograd --------------------------------------------------------------------------------------------------------------
def net_layers():
    net = tc.trunk_net()
    blk = net['stages'][1][0]                      # body.layer2.0: conv2 carries the stride, downsample.0 is the strided 1x1
    return dict(conv1=blk['conv1'], conv2=blk['conv2'], conv3=blk['conv3'], down=blk['down'], inner=net['inner'][1], outer=net['outer'][1])


# (layer, (H, W) of dX, add rule or None, mask)
LAUNCHES = [('conv2', (5, 7), None, True), ('conv2', (4, 6), None, True), ('conv1', (5, 7), r16.SAME, True), ('conv1', (5, 7), r16.EVEN, True),
            ('outer', (3, 4), r16.NEAREST_T, False), ('inner', (4, 6), None, True), ('conv3', (2, 1), None, False)]


def launch_data(case):
    name, (H, W), rule, mask = case
    layer = net_layers()[name]
    rng = np.random.RandomState(sum(map(ord, name)) + H * 16 + W + (0 if rule is None else len(rule)))
    w = layer['weight']
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    stride = layer['stride']
    ws = r16.ws16(w, layer['scale'])
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = exact(rng, (2, O, Ho, Wo))
    add_hw = {None: None, r16.SAME: (H, W), r16.EVEN: ((H - 1) // 2 + 1, (W - 1) // 2 + 1), r16.NEAREST_T: (2 * H - 1, 2 * W)}[rule]
    adds = [] if rule is None else [(rule, exact(rng, (2, C) + add_hw))]
    v = exact(rng, (2, C, H, W))
    v[rng.uniform(0, 1, v.shape) < 0.2] = 0
    return ws, stride, k, g, adds, v if mask else None


@pytest.mark.parametrize('case', LAUNCHES, ids=lambda c: f'{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-{"mask" if c[3] else "plain"}')
def test_the_launch_evaluation_is_autograds(case):
    ws, stride, k, g, adds, y = launch_data(case)
    H, W = case[1]
    d = r16.dgrad64(ws, stride, g, H, W, adds, y)
    v = t64(np.ones((2, ws.shape[1], H, W)) if y is None else y).requires_grad_()
    yv = v if y is None else torch.relu(v)          # y = relu(v): y <= 0 exactly where v <= 0
    loss = (F.conv2d(yv, t64(ws), None, stride, k // 2) * t64(g)).sum()
    for rule, r in adds:
        if rule == r16.SAME:
            loss = loss + (yv * t64(r)).sum()
        elif rule == r16.EVEN:
            loss = loss + (yv[..., ::2, ::2] * t64(r)).sum()
        else:
            loss = loss + (F.interpolate(yv, size=r.shape[2:], mode='nearest') * t64(r)).sum()
    loss.backward()
    got = np.where(d['blocked'], 0.0, d['t64'])
    err, top = float(np.abs(got - v.grad.numpy()).max()), float(np.abs(got).max())
    print(f'{case[0]}: max |err| = {err:.3e} of {top:.3e}')
    assert err <= 1e-12 * top
    assert (d['K'] >= ws.shape[0]).all() and (d['K'] <= ws.shape[0] * k * k).all() and (d['S'] >= np.abs(d['t64']) * (1 - 1e-12)).all()
    if adds and adds[0][0] == r16.EVEN:
        assert set(np.unique(d['n'])) == {0.0, 1.0} and d['n'][0, 0, 1, 1] == 0 and d['n'][0, 0, 0, 0] == 1
    if adds and adds[0][0] == r16.NEAREST_T:
        assert d['n'].sum() == d['n'].shape[0] * d['n'].shape[1] * adds[0][1].shape[2] * adds[0][1].shape[3]
    # the bounds hold on a float32 emulation and are not vacuous: the emulation's error is a visible share of them
    emu = r16.dgrad_f32(ws, stride, g, H, W, adds, y)
    b32, b16 = r16.dgrad_bound(d)
    live = ~d['blocked']
    e = np.abs(emu.astype(np.float64) - d['t64'])
    assert (e[live] <= b16[live]).all() and not emu[d['blocked']].any() and not np.signbit(emu[d['blocked']]).any()
    share = float((e[live] / np.maximum(b16[live], 1e-300)).max())
    print(f'{case[0]}: the emulation uses {share:.3f} of the bfloat16 bound')
    assert share > 1e-3                           # a bound a thousand times the error of a correct float32 accumulation would tell nothing
    assert (b16 >= b32).all() and (b32[d['S'] > 0] > 0).all()


@pytest.mark.parametrize('name', ['conv2', 'down', 'outer', 'inner'])
def test_the_weight_gradient_evaluation_is_conv2ds(name):
    layer = net_layers()[name]
    w = layer['weight']
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    stride = layer['stride']
    rng = np.random.RandomState(len(name) + O)
    x = exact(rng, (2, C, 5, 7))
    g = exact(rng, (2, O, (5 - 1) // stride + 1, (7 - 1) // stride + 1))
    wg = r16.wgrad64(k, stride, layer['scale'], x, g, bias=layer['scale'] is None)
    wt = torch.zeros(O, C, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(O, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(t64(x), wt, b, stride, k // 2)
    if layer['scale'] is not None:
        out = out * t64(layer['scale']).reshape(1, -1, 1, 1)
    out.backward(t64(g))
    assert np.abs(wg['dW'] - wt.grad.numpy()).max() <= 1e-12 * np.abs(wg['dW']).max()
    if layer['scale'] is None:
        assert np.abs(wg['db'] - b.grad.numpy()).max() <= 1e-12 * np.abs(wg['db']).max()
    else:
        assert wg['db'] is None
    bw, bb = r16.wgrad_bound16(wg)
    assert (bb is None) == (wg['db'] is None)
    emu = r16.wgrad_f32(k, stride, layer['scale'], x, g)
    e = np.abs(emu.astype(np.float64) - wg['dW'])
    assert (e <= bw).all()
    share = float((e / np.maximum(bw, 1e-300)).max())
    print(f'{name}: T = {wg["T"]}, the emulation uses {share:.3f} of the bound')
    assert share > 1e-3


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------------
def test_train_dtype_refuses_before_it_touches_a_device():
    from cosypose_amd import Detector, DetectorTrunk
    sd = bc.torch_sd()
    with pytest.raises(ValueError, match='loss scaler'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float16)
    with pytest.raises(ValueError, match='loss scaler'):
        Detector.from_state_dict(sd, tc.E2E_LABELS, trainable=True, train_dtype=torch.float16)
    for td in (torch.bfloat16, torch.float32):
        with pytest.raises(ValueError, match='trainable=True'):
            DetectorTrunk.from_state_dict(sd, train_dtype=td)
        with pytest.raises(ValueError, match='trainable=True'):
            Detector.from_state_dict(sd, tc.E2E_LABELS, train_dtype=td)
    for td in (torch.float64, torch.int8, 'bfloat16'):
        with pytest.raises(ValueError, match='train_dtype must be'):
            DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_dtype=td)
    with pytest.raises(ValueError, match='float32 only'):                            # dtype stays the parameters' type: the master weights
        DetectorTrunk.from_state_dict(sd, dtype=torch.bfloat16, device='cuda', trainable=True, train_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='ROCm device'):
        DetectorTrunk.from_state_dict(sd, trainable=True, train_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='stem'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=0, train_dtype=torch.bfloat16)
    assert DetectorTrunk.from_state_dict(sd).train_dtype is None


def test_the_bfloat16_exports_are_bound_with_the_headers_arity():
    import cosypose_amd
    from cosypose_amd import _lib
    want = {'cosy_trunk_weight_pack16': 10, 'cosy_trunk_grad_pack16': 6, 'cosy_trunk_dgrad16': 12, 'cosy_trunk_wgrad16': 9}
    for name, n in want.items():
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][0]) == n and _lib._SIGNATURES[name][1] is _lib._I, name
    for name in ('check_train_dtype', 'trunk_grad_pack'):
        assert getattr(cosypose_amd.detector_trunk_backward, name) is not None

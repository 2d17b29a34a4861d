"""The twin of the heads' bfloat16 backward (tests/detheadbwd16_ref.py): both packing rules for siblings and for the
deconvolution against a dense loop and against the host packing of w.to(bfloat16), the gradient pack's pad and column order, its float64 launch
evaluations against torch.autograd in float64 on the three heads of dethead_case.torch_heads fed bf16-exact tensors, its bounds on a
float32-accumulate emulation, and what train_dtype= / heads_train_dtype= refuse before they touch a device.  CPU only;
tests/test_detector_heads_backward16.py holds the kernels against the twin."""
import numpy as np
import pytest
import torch

import dethead_case as fc
import dethead_ref as ref
import detheadbwd16_ref as r16

F32 = np.float32


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def exact(rng, shape, spread=1.0):
    return r16.bf16(rng.normal(0, spread, shape).astype(F32))


def head_layers():
    hw = fc.head_weights()
    return dict(rpn=ref.rpn_layers(hw), box=ref.box_layers(hw), mask=ref.mask_layers(hw))


# ---- packings ----------------------------------------------------------------------------------------------------------------------------
def pack_layers():
    h = head_layers()
    rng = np.random.RandomState(4)
    wide = dict(kind='linear', weight=rng.normal(0, 1, (70, 40)).astype(F32), bias=rng.normal(0, 1, 70).astype(F32), relu=False)      # two row tiles of 64, two k-blocks
    return [('rpn siblings 3 + 12', h['rpn'][1], 3), ('box siblings 3 + 12', h['box'][2], 3), ('deconv', h['mask'][4], None), ('3x3', h['mask'][0], None),
            ('fc6', h['box'][0], None), ('linear 40 -> 70', wide, None)]


@pytest.mark.parametrize('name,layer,n_split', pack_layers(), ids=[p[0] for p in pack_layers()])
def test_both_packing_rules_are_the_dense_loops_and_the_host_packings_bytes(name, layer, n_split):
    from cosypose_amd.detector_heads import HeadLayer, pack_weight, transposed_weight
    w, kind = np.asarray(layer['weight'], F32), layer['kind']
    for which, op, packed in (('fwd', r16.fwd_operand(layer), r16.pack_fwd16(layer)), ('bwd', r16.bwd_operand(layer), r16.pack_bwd16(layer))):
        N, T, K = op.shape
        assert r16.is_bf16(op) and packed.dtype == np.uint16 and packed.size == (-(-N // 64) * 64) * T * (-(-K // 32) * 32), which
        dense = np.array([r16.pack16_at(op, i) for i in range(packed.size)], F32)
        assert np.array_equal(r16.from_bits(packed).view(np.uint32), dense.view(np.uint32)), which
    wb, fo, bo = r16.bf16(w), r16.fwd_operand(layer), r16.bwd_operand(layer)
    if kind == 'deconv':                           # forward rows (o, dy, dx), one tap; backward taps (dy, dx) ascending, rows c, reduction o
        C, O = w.shape[:2]
        assert fo.shape == (4 * O, 1, C) and bo.shape == (C, 4, O)
        assert fo[4 * 5 + 2 * 1 + 0, 0, 3] == wb[3, 5, 1, 0] and bo[3, 2 * 1 + 0, 5] == wb[3, 5, 1, 0] and bo[7, 1, 2] == wb[7, 2, 0, 1]
        host = HeadLayer.deconv(torch.from_numpy(w), torch.from_numpy(layer['bias']), dtype=torch.bfloat16)
    elif kind == 'conv':                           # the taps of the backward operand run in reverse
        k = w.shape[2]
        assert fo[2, k * k - 1, 5] == wb[2, 5, k - 1, k - 1] and bo[5, 0, 2] == wb[2, 5, k - 1, k - 1] and bo[5, k * k - 1, 2] == wb[2, 5, 0, 0]
        host = HeadLayer.conv(torch.from_numpy(w), torch.from_numpy(layer['bias']), dtype=torch.bfloat16)
    else:
        assert fo[2, 0, 5] == wb[2, 5] and bo[5, 0, 2] == wb[2, 5]
        host = HeadLayer.linear(torch.from_numpy(w), torch.from_numpy(layer['bias']), dtype=torch.bfloat16)
    if n_split is not None:                         # siblings: w0's outputs, then w1's, in both packings
        pair = [(torch.from_numpy(w[:n_split]), torch.from_numpy(layer['bias'][:n_split])), (torch.from_numpy(w[n_split:]), torch.from_numpy(layer['bias'][n_split:]))]
        host = HeadLayer.siblings(pair[0], pair[1], kind, dtype=torch.bfloat16)
        assert host.n_split == n_split
    u16 = lambda t: t.view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(u16(host.packed), r16.pack_fwd16(layer)), 'the host packing of w.to(bfloat16)'
    assert np.array_equal(host.packed_bias.numpy().view(np.uint32), r16.bias_pad(layer).view(np.uint32))
    back = pack_weight(transposed_weight(kind, torch.from_numpy(w)), torch.bfloat16)
    assert np.array_equal(u16(back), r16.pack_bwd16(layer)), 'the host packing of the transposed weight rounded to bfloat16'


def test_the_gradient_pack_puts_g0_then_g1_then_zeros():
    rng = np.random.RandomState(8)
    g0, g1 = rng.normal(0, 1, (2, 3, 2, 5)).astype(F32), rng.normal(0, 1, (2, 12, 2, 5)).astype(F32)
    g0[0, 0, 0, :3] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0]
    rows = r16.grad_rows(g0, g1)
    assert rows.shape == (20, 16) and rows.dtype == np.uint16 and not rows[:, 15].any()
    assert rows[0, 0] == 0x3F80 and rows[1, 0] == 0x3F82 and rows[2, 0] == 0x8000            # ties to even; the sign of a zero is kept
    v = r16.from_bits(rows)
    for b, y, x in ((0, 0, 0), (1, 1, 4), (0, 1, 2)):
        r = (b * 2 + y) * 5 + x
        assert np.array_equal(v[r, :3], r16.bf16(g0[b, :, y, x])) and np.array_equal(v[r, 3:15], r16.bf16(g1[b, :, y, x]))
    assert r16.grad_rows(g1).shape == (20, 16) and r16.grad_rows(g0[:, :, 0, 0][:, :, None]).shape == (2, 8)
    assert np.array_equal(r16.grad_rows(g0, np.zeros_like(g1))[:, :3], rows[:, :3]) and not r16.grad_rows(g0, np.zeros_like(g1))[:, 3:].any()


# ---- the launch evaluations against autograd -------------------------------------------------------------------------------------------------
def torch_chain(mods, name, x):
    """the torch.nn heads of dethead_case in float64 on x -> the raw outputs as one tensor with the twin's column order"""
    rpn, box_head, box_pred, mask_head, mask_pred = mods
    if name == 'rpn':
        obj, dlt = rpn([x])
        return torch.cat([obj[0], dlt[0]], 1)
    if name == 'box':
        return torch.cat(box_pred(box_head(x)), 1)
    return mask_pred(mask_head(x))


@pytest.mark.parametrize('name', ['rpn', 'box', 'mask'])
def test_the_launch_evaluations_chain_to_autograds_gradients(name):
    """every launch of a head re-walked in float64 from bf16-exact operands, the masks from the float64 forward: the chain of the twin's launch
    evaluations is torch.autograd's backward of the same modules holding the bf16-exact weights"""
    hw16 = {k: (r16.bf16(v) if k.endswith('.weight') else v) for k, v in fc.head_weights().items()}
    layers = [r16.layer16(l) for l in head_layers()[name]]
    mods = fc.torch_heads(hw16, torch.float64)
    for m in mods:
        m.requires_grad_(True)
    feats, roi, mroi = fc.head_inputs()
    x = r16.bf16({'rpn': feats[0], 'box': roi.reshape(len(roi), -1), 'mask': mroi}[name])
    xt = t64(x if name != 'box' else x.reshape(roi.shape)).requires_grad_()
    out = torch_chain(mods, name, xt)
    rng = np.random.RandomState(len(name))
    g = exact(rng, tuple(out.shape))
    out.backward(t64(g))
    acts = [np.asarray(x, np.float64)]
    for layer in layers:
        acts.append(ref.layer64(layer, acts[-1])[0])
    params = {'rpn': [('rpn.head.conv', None), ('rpn.head.cls_logits', 'rpn.head.bbox_pred')],
              'box': [('roi_heads.box_head.fc6', None), ('roi_heads.box_head.fc7', None), ('roi_heads.box_predictor.cls_score', 'roi_heads.box_predictor.bbox_pred')],
              'mask': [(f'roi_heads.mask_head.mask_fcn{i}', None) for i in range(1, 5)] + [('roi_heads.mask_predictor.conv5_mask', None),
                                                                                           ('roi_heads.mask_predictor.mask_fcn_logits', None)]}[name]
    named = {f'{prefix}.{k}': p for prefix, m in zip(('rpn.head', 'roi_heads.box_head', 'roi_heads.box_predictor', 'roi_heads.mask_head', 'roi_heads.mask_predictor'), mods)
             for k, p in m.named_parameters()}
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)
    for i in range(len(layers) - 1, -1, -1):
        wg = r16.wgrad64(layers[i], acts[i], g)
        first, second = params[i]
        n = named[first + '.weight'].shape[1 if layers[i]['kind'] == 'deconv' else 0]
        assert close(wg['dW'][:n] if second else wg['dW'], named[first + '.weight'].grad.numpy()) and close(wg['db'][:n], named[first + '.bias'].grad.numpy()), first
        if second:
            assert close(wg['dW'][n:], named[second + '.weight'].grad.numpy()) and close(wg['db'][n:], named[second + '.bias'].grad.numpy()), second
        cells = int(np.prod(acts[i].shape) // acts[i].shape[1])
        assert wg['T_W'] == cells and wg['T_b'] == (4 * cells if layers[i]['kind'] == 'deconv' else cells)
        d = r16.dgrad64(layers[i], g, acts[i] if i and layers[i - 1].get('relu') else None)
        taps = 4 if layers[i]['kind'] == 'deconv' else int(np.prod(np.shape(layers[i]['weight'])[2:]))
        assert d['K'] == taps * g.shape[1] and (d['S'] >= np.abs(d['t64']) * (1 - 1e-12)).all()
        g = np.where(d['blocked'], 0.0, d['t64'])                              # what the launch stores, before its rounding
    assert close(g.reshape(xt.shape), xt.grad.numpy())


# ---- the bounds on a float32-accumulate emulation ---------------------------------------------------------------------------------------------
EMU_CASES = [('conv3', 8, 24, True, 2, 5, 7), ('conv1', 40, 15, False, 2, 5, 7), ('linear', 392, 15, False, 65, 1, 1), ('deconv', 16, 8, True, 1, 4, 6)]


@pytest.mark.parametrize('c', EMU_CASES, ids=fc.case_id)
def test_the_bounds_hold_on_a_float32_emulation_and_are_not_vacuous(c):
    import detheadbwd_case as bc
    layer, x = fc.case_data(c)
    layer, x, g = r16.layer16(layer), r16.bf16(x), r16.bf16(bc.case_grad(c))
    y = r16.bf16(np.where(np.abs(x) < 0.3, 0, x).astype(F32))
    d = r16.dgrad64(layer, g, y)
    b, b16 = r16.dgrad_bound(d)
    live = ~d['blocked']
    assert d['blocked'].any() and live.any() and (b16 >= b).all() and (b[d['S'] > 0] > 0).all()
    for rows, bound in ((True, b16), (False, b)):
        emu = r16.dgrad_f32(layer, g, y, rows)
        e = np.abs(emu.astype(np.float64) - d['t64'])
        assert (e[live] <= bound[live]).all() and not emu[d['blocked']].any() and not np.signbit(emu[d['blocked']]).any()
        share = float((e[live] / np.maximum(bound[live], 1e-300)).max())
        print(f'{fc.case_id(c)}: the {"row" if rows else "NCHW"} emulation uses {share:.4f} of its bound')
        assert share > (1e-3 if rows else 1e-4)      # a bound thousands of times the error of a correct float32 accumulation would tell nothing
    wg = r16.wgrad64(layer, x, g)
    bW, bb = r16.wgrad_bound(wg)
    dW, db = r16.wgrad_f32(layer, x, g)
    M = x.shape[0] * (1 if x.ndim == 2 else x.shape[2] * x.shape[3])
    assert wg['T_W'] == M and wg['T_b'] == (4 * M if c[0] == 'deconv' else M)      # the deconvolution's bias sums the rows of g
    for part, emu, want, bound in (('dW', dW, wg['dW'], bW), ('db', db, wg['db'], bb)):
        assert emu.shape == want.shape, part
        e = np.abs(emu.astype(np.float64) - want)
        assert (e <= bound).all(), part
        share = float((e / np.maximum(bound, 1e-300)).max())
        print(f'{fc.case_id(c)}: T = {wg["T_" + part[1]]}, the {part} emulation uses {share:.4f} of its bound')
        assert share > 1e-4 or part == 'db', part        # db: float32 adds a few hundred 8-bit significands of one scale exactly, on the device too


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------------
def test_train_dtype_and_heads_train_dtype_refuse_before_they_touch_a_device():
    import dettrunk_case as tc
    import dettrunkbwd_case as tbc
    from cosypose_amd import Detector, DetectorHeads
    sd = {k: torch.from_numpy(v) for k, v in fc.head_weights().items()}
    mods = fc.torch_heads()
    with pytest.raises(ValueError, match='loss scaler'):
        DetectorHeads.from_state_dict(sd, device='cuda', trainable=True, train_dtype=torch.float16)
    with pytest.raises(ValueError, match='loss scaler'):
        DetectorHeads.from_modules(*mods, device='cuda', trainable=True, train_dtype=torch.float16)
    for td in (torch.bfloat16, torch.float32):
        with pytest.raises(ValueError, match='trainable=True'):
            DetectorHeads.from_state_dict(sd, train_dtype=td)
        with pytest.raises(ValueError, match='trainable=True'):
            DetectorHeads.from_modules(*mods, train_dtype=td)
    for td in (torch.float64, torch.int8, 'bfloat16'):
        with pytest.raises(ValueError, match='train_dtype must be'):
            DetectorHeads.from_state_dict(sd, device='cuda', trainable=True, train_dtype=td)
    with pytest.raises(ValueError, match='trainable heads are float32 only'):          # dtype stays the parameters' type: its present refusal
        DetectorHeads.from_state_dict(sd, dtype=torch.bfloat16, device='cuda', trainable=True)
    with pytest.raises(ValueError, match='trainable heads are float32 only'):
        DetectorHeads.from_state_dict(sd, dtype=torch.bfloat16, device='cuda', trainable=True, train_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='ROCm device'):
        DetectorHeads.from_state_dict(sd, trainable=True, train_dtype=torch.bfloat16)
    assert DetectorHeads.from_state_dict(sd).train_dtype is None
    full = tbc.torch_sd()
    with pytest.raises(ValueError, match='loss scaler'):
        Detector.from_state_dict(full, tc.E2E_LABELS, trainable=True, heads_train_dtype=torch.float16)
    with pytest.raises(ValueError, match='loss scaler'):
        Detector.from_state_dict(full, tc.E2E_LABELS, trainable=True, train_dtype=torch.bfloat16, heads_train_dtype=torch.float16)
    with pytest.raises(ValueError, match='trainable=True'):
        Detector.from_state_dict(full, tc.E2E_LABELS, heads_train_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='train_dtype must be'):
        Detector.from_state_dict(full, tc.E2E_LABELS, trainable=True, heads_train_dtype=torch.float64)


def test_the_bfloat16_exports_are_bound_with_the_headers_arity():
    import cosypose_amd
    from cosypose_amd import _lib
    want = {'cosy_head_weight_pack16': 12, 'cosy_head_grad_pack16': 8, 'cosy_head_dgrad16': 3, 'cosy_head_wgrad16': 9}
    for name, n in want.items():
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][0]) == n and _lib._SIGNATURES[name][1] is _lib._I, name
    assert cosypose_amd.detector_heads.TrainableLayer.dtype == torch.float32                    # the class default stays section 28's

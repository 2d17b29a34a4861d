"""The CPU half of DESIGN.md section 28: the twin tests/detheadbwd_ref.py against torch.autograd in float64 (single layers and the three
heads of dethead_case.torch_heads), the twin's float32 chain against its own float64 sum, the index rule of the transposed packing, and the
refusals that need no device.  Running every case here is also what holds detheadbwd_case.SALT: a DoubleRounding would raise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dethead_case as fc
import dethead_ref as ref
import detheadbwd_case as bc
import detheadbwd_ref as bref
from cosypose_amd import detector_heads as dh

f64 = torch.float64


def autograd64(layer, x, g):
    """-> dX, dW, db of one twin layer by torch.autograd in float64 (no ReLU: g is the pre-activation gradient)"""
    w = torch.tensor(np.asarray(layer['weight'], np.float64), requires_grad=True)
    b = torch.tensor(np.asarray(layer['bias'], np.float64), requires_grad=True)
    xx = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    if layer['kind'] == 'linear':
        y = F.linear(xx, w, b)
    elif layer['kind'] == 'conv':
        y = F.conv2d(xx, w, b, padding=w.shape[2] // 2)
    else:
        y = F.conv_transpose2d(xx, w, b, stride=2)
    y.backward(torch.tensor(np.asarray(g, np.float64)))
    return xx.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def close(a, b, what):
    scale = 1 + np.abs(b).max() if b.size else 1
    assert a.shape == b.shape and np.abs(a - b).max(initial=0) <= 1e-11 * scale, what


@pytest.mark.parametrize('case', bc.CASES, ids=bc.case_id)
def test_twin_layer_equals_autograd_in_float64(case):
    layer, x = fc.case_data(case)
    g, w = bc.case_grad(case), bc.want(case)
    dx, dW, db = autograd64(layer, x, g)
    close(w['dx64'], dx, 'dX')
    close(w['dW'], dW, 'dW')
    close(w['db'], db, 'db')
    assert w['T_W'] == (x.shape[0] if layer['kind'] == 'linear' else x.shape[0] * x.shape[2] * x.shape[3])
    assert w['T_b'] == (4 if layer['kind'] == 'deconv' else 1) * w['T_W']
    # the float32 chain against the float64 sum: K = the reduction length (taps x outputs) fmaf terms, no bias add
    rows, wt, back = bref.dgrad_operands(layer, g.astype(np.float64))
    M, T, O = rows.shape
    S = back(np.abs(rows).reshape(M, T * O) @ np.abs(wt.astype(np.float64)).reshape(-1, T * O).T)
    assert w['dx32'].dtype == np.float32 and (np.abs(w['dx32'] - w['dx64']) <= (T * O + 2) * bref.U32 * S).all()


def test_twin_heads_equal_autograd_in_float64():
    sd, (feats, roi, mroi), g = fc.head_weights(), fc.head_inputs(), bc.head_grads()
    rpn, box, pred, mask, mpred = (m.double().requires_grad_(True) for m in fc.torch_heads())
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    # RPN, level by level
    want = {}
    for l, (f, gl) in enumerate(zip(feats, g['rpn'])):
        x = t(f)
        o, d = rpn([x])
        torch.cat([o[0], d[0]], 1).backward(torch.tensor(gl.astype(np.float64)))
        dx, (conv, pr) = bref.head_backward(ref.rpn_layers(sd), f, gl, exact=True)
        close(dx, x.grad.numpy(), f'rpn dX level {l}')
        for k, v in (('conv', conv), ('pred', pr)):
            want[k] = v if k not in want else bc.add(want[k], v)
    cls, bb = bc.split(want['pred'], fc.A)
    for m, d in ((rpn.conv, want['conv']), (rpn.cls_logits, cls), (rpn.bbox_pred, bb)):
        close(d['dW'], m.weight.grad.numpy(), 'rpn dW')
        close(d['db'], m.bias.grad.numpy(), 'rpn db')
    # box head
    x = t(roi)
    torch.cat(pred(box(x)), 1).backward(torch.tensor(g['box'].astype(np.float64)))
    dx, (fc6, fc7, pr) = bref.head_backward(ref.box_layers(sd), roi.reshape(len(roi), -1), g['box'], exact=True)
    close(dx.reshape(roi.shape), x.grad.numpy(), 'box dX')
    cls, bb = bc.split(pr, fc.K)
    for m, d in ((box.fc6, fc6), (box.fc7, fc7), (pred.cls_score, cls), (pred.bbox_pred, bb)):
        close(d['dW'], m.weight.grad.numpy(), 'box dW')
        close(d['db'], m.bias.grad.numpy(), 'box db')
    # mask head
    x = t(mroi)
    mpred(mask(x)).backward(torch.tensor(g['mask'].astype(np.float64)))
    dx, grads = bref.head_backward(ref.mask_layers(sd), mroi, g['mask'], exact=True)
    close(dx, x.grad.numpy(), 'mask dX')
    mods = [getattr(mask, f'mask_fcn{i}') for i in range(1, 5)] + [mpred.conv5_mask, mpred.mask_fcn_logits]
    for m, d in zip(mods, grads):
        close(d['dW'], m.weight.grad.numpy(), 'mask dW')
        close(d['db'], m.bias.grad.numpy(), 'mask db')


def test_whole_head_chains_raise_no_double_rounding():
    wants = bc.head_wants()
    assert [d.dtype for d in wants['rpn'][0]] == [np.float32] * 3 and wants['box'][0].dtype == np.float32 and wants['mask'][0].dtype == np.float32
    assert all(np.isfinite(dx).all() for dx in wants['rpn'][0] + [wants['box'][0], wants['mask'][0]])


def test_relu_mask_rule():
    y = np.array([-1.0, -0.0, 0.0, 1e-30, np.nan, 2.0], np.float32)
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0, np.nan], np.float32)
    out = bref.relu_mask(y, v)
    assert np.array_equal(out[:5], np.array([0, 0, 0, 4, 5], np.float32)) and np.isnan(out[5])
    ty = torch.tensor(y, dtype=f64, requires_grad=True)
    torch.relu(ty).backward(torch.tensor(v[:4].tolist() + [5.0, 7.0], dtype=f64))
    assert ty.grad.tolist()[:4] == [0, 0, 0, 4]                                 # torch's threshold_backward on the same y (relu(y) <= 0 where y <= 0)


@pytest.mark.parametrize('kind,shape', [('conv', (5, 24, 3, 3)), ('conv', (3, 8, 1, 1)), ('linear', (19, 40)), ('deconv', (24, 8, 2, 2))])
def test_transposed_packing_index_rule(kind, shape):
    """element [nt][tap][kb][lane][e] of the backward packing holds w[o][c] at the flipped tap with c = 16 nt + (lane & 15) (the GEMM's row) and
    o = 16 kb + 4 (lane >> 4) + e (its reduction index); zero where c or o does not exist"""
    w = torch.from_numpy(np.random.RandomState(3).normal(0, 1, shape).astype(np.float32))
    wt = dh.transposed_weight(kind, w)
    C, taps, O = wt.shape
    assert (C, O) == ((shape[1], shape[0]) if kind != 'deconv' else (shape[0], shape[1])) and taps == (1 if kind == 'linear' else 4 if kind == 'deconv' else shape[2] * shape[2])
    packed = dh.pack_weight(wt, torch.float32).numpy()
    KBn, NP = -(-O // 16), -(-C // 64) * 64
    assert packed.shape == (NP * taps * KBn * 16,)
    p = packed.reshape(NP // 16, taps, KBn, 64, 4)
    wn = w.numpy()
    for nt in range(NP // 16):
        for tap in range(taps):
            for kb in range(KBn):
                for lane in range(64):
                    for e in range(4):
                        c, o = 16 * nt + (lane & 15), 16 * kb + 4 * (lane >> 4) + e
                        if c >= C or o >= O:
                            v = 0.0
                        elif kind == 'linear':
                            v = wn[o, c]
                        elif kind == 'conv':
                            k = shape[2]
                            ft = taps - 1 - tap
                            v = wn[o, c, ft // k, ft % k]
                        else:
                            v = wn[c, o, tap >> 1, tap & 1]
                        assert p[nt, tap, kb, lane, e] == np.float32(v), (nt, tap, kb, lane, e)


def test_refusals_that_need_no_device():
    sd = {k: torch.from_numpy(v) for k, v in fc.head_weights().items()}
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match='float32 only'):
            dh.DetectorHeads.from_state_dict(sd, dtype=dtype, trainable=True)
        with pytest.raises(ValueError, match='float32 only'):
            dh.DetectorHeads.from_modules(*fc.torch_heads(), dtype=dtype, trainable=True)
    with pytest.raises(ValueError, match='device'):
        dh.DetectorHeads.from_state_dict(sd, trainable=True)                   # CPU weights and no device: there is no CPU path
    with pytest.raises(ValueError, match='device'):
        dh.TrainableLayer.linear(torch.zeros(3, 8), torch.zeros(3), device='cpu')
    plain = dh.DetectorHeads.from_state_dict(sd)
    assert plain.trainable is False and plain.rpn_head.parameters() == []
    for call in (plain.parameters, plain.named_parameters, plain.state_dict, lambda: plain.load_state_dict(sd)):
        with pytest.raises(RuntimeError, match='inference only'):
            call()
    with pytest.raises(ValueError, match='TrainableLayer'):
        dh.layer_backward(plain.box_head.fc6, torch.zeros(1, 392), torch.zeros(1, 24))
    with pytest.raises(ValueError, match='kind'):
        dh.transposed_weight('pool', torch.zeros(1, 8))

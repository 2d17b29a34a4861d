"""The twin of the trunk's backward (tests/dettrunkbwd_ref.py) against torch.autograd in float64, its index rules against
torch's own, and what the trainable trunk refuses before it touches a device.  CPU only; tests/test_detector_trunk_backward.py holds the
kernels against the twin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dettrunk_case as tc
import dettrunkbwd_case as bc
import dettrunkbwd_ref as ref

F32 = np.float32


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def close(name, got, want, tol=1e-10):
    """within tol of the tensor's largest magnitude: both sides are float64 sums of at most a few thousand terms in different orders, about
    n 2^-53 = 1e-12 of it; the factor 100 is margin"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f'{name}: max |err| = {err:.3e} of {top:.3e}')
    assert err <= tol * max(top, 1e-300), name


# ---- the whole chain against autograd --------------------------------------------------------------------------------------------------
def reference_requires_grad(m, train_from_stage):
    """the reference's set: body.layer{train_from_stage}.. and the FPN; conv1, the stages below and every FrozenBatchNorm hold none"""
    names = []
    for k, p in m.named_parameters():
        stage = int(k.split('.')[1][5:]) if k.startswith('body.layer') else None
        if k.startswith('fpn.') or (stage is not None and stage >= train_from_stage):
            p.requires_grad_(True)
            names.append(k)
    return names


@pytest.mark.parametrize('shape', tc.INPUTS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('train_from_stage', [2, 1])
def test_the_exact_twin_is_autograds_backward(shape, train_from_stage):
    m = tc.torch_trunk().double()
    names = reference_requires_grad(m, train_from_stage)
    assert names and all(('conv' in k or 'downsample.0' in k or k.startswith('fpn.')) for k in names)
    images = tc.trunk_images(shape)
    net = tc.trunk_net()
    rng = np.random.RandomState(3)
    seen = {}

    def cut(mod, inp):                             # the first trainable stage's input is no parameter's function: make it a leaf that keeps its gradient
        seen['x'] = inp[0].detach().requires_grad_()
        return (seen['x'],)
    hook = getattr(m.body, f'layer{train_from_stage}').register_forward_pre_hook(cut)
    x = t64(images)
    out = m(x)
    hook.remove()
    grads = [rng.normal(0, 1, tuple(o.shape)) for o in out]
    torch.autograd.backward(out, [t64(g) for g in grads])
    got = ref.trunk_backward(net, images, grads, train_from_stage, exact=True, input_grad=True)
    assert set(got['params']) == {k[:-7] for k in names if k.endswith('.weight')}
    for k in names:
        p = dict(m.named_parameters())[k]
        d = got['params'][k.rsplit('.', 1)[0]]
        close(k, d['dW'] if k.endswith('.weight') else d['db'], p.grad.numpy())
    close('the gradient at the first trainable block\'s input', got['dx'], seen['x'].grad.numpy())


def test_a_later_first_stage_names_a_subset_of_the_same_chain():
    shape = tc.INPUTS[1]
    full = bc.trunk_want(shape, 1)
    for tfs in (2, bc.N_STAGES + 1):
        part = ref.trunk_backward(tc.trunk_net(), tc.trunk_images(shape), bc.trunk_grads(shape), tfs, keep=bc.trunk_forward(shape))
        assert set(part['params']) == {k for k in full['params'] if bc.trained(k, tfs)}
        assert set(part['rows']) == {k for k in full['rows'] if bc.trained(k, tfs)}
        for k, v in part['rows'].items():
            assert np.array_equal(v.view(np.int32), full['rows'][k].view(np.int32)), k
        for k, v in part['params'].items():
            assert np.array_equal(v['dW'], full['params'][k]['dW']), k


# ---- index rules --------------------------------------------------------------------------------------------------------------------------
def test_nearest_t_is_the_transpose_of_torchs_nearest():
    for n_in in range(1, 65):
        for n_out in (2 * n_in - 1, 2 * n_in):
            if n_out < 1:
                continue
            cells = ref.nearest_t_cells(n_in, n_out)
            up = F.interpolate(torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in), size=(1, n_out), mode='nearest').reshape(-1).long().numpy()
            want = [np.flatnonzero(up == c) for c in range(n_in)]
            for c, (lo, hi) in enumerate(cells):
                assert list(range(lo, hi)) == list(want[c]), (n_in, n_out, c)
            assert sum(hi - lo for lo, hi in cells) == n_out


def test_nearest_t_add_is_interpolates_backward():
    rng = np.random.RandomState(1)
    for (H, W), (fH, fW) in (((3, 4), (5, 7)), ((3, 5), (6, 10)), ((2, 2), (3, 4))):
        r = rng.normal(0, 1, (2, 8, fH, fW))
        coarse = torch.zeros(2, 8, H, W, dtype=torch.float64, requires_grad=True)
        F.interpolate(coarse, size=(fH, fW), mode='nearest').backward(t64(r))
        got = ref.apply_adds(np.zeros((2, 8, H, W)), [(ref.NEAREST_T, r)], np.float64)
        close(f'{fH}x{fW} -> {H}x{W}', got, coarse.grad.numpy(), 1e-14)


@pytest.mark.parametrize('H,W', bc.MAPS)
@pytest.mark.parametrize('k', [3, 1])
def test_the_strided_data_gradient_and_the_even_rule_are_conv2ds_backward(H, W, k):
    rng = np.random.RandomState(H * 10 + W + k)
    layer = dict(weight=rng.normal(0, 1, (16, 8, k, k)).astype(F32), stride=2, scale=rng.uniform(0.5, 1.5, 16).astype(F32), bias=np.zeros(16, F32), relu=False)
    x = torch.zeros(2, 8, H, W, dtype=torch.float64, requires_grad=True)
    ws = t64(ref.ws_of(layer, exact=True))
    out = F.conv2d(x, ws, None, 2, k // 2)
    g = rng.normal(0, 1, tuple(out.shape))
    out.backward(t64(g))
    if k == 3:                                     # the four parity classes: 1, 2, 2 or 4 live taps, an even H's last row reads past the output map
        got = ref.dx64(layer, g, H, W)
    else:                                          # downsample.0: a stride-1 gradient on the output grid, entering through EVEN
        d = ref.dx64(ref.on_output_grid(layer), g, *g.shape[2:])
        got = ref.apply_adds(np.zeros((2, 8, H, W)), [(ref.EVEN, d)], np.float64)
    close(f'k{k} {H}x{W}', got, x.grad.numpy(), 1e-13)


def test_the_even_rule_leaves_an_odd_cells_negative_zero():
    t = np.full((1, 8, 3, 3), -0.0, F32)
    got = ref.apply_adds(t, [(ref.EVEN, np.zeros((1, 8, 2, 2), F32))], F32)
    assert np.signbit(got[0, 0, 1, 1]) and np.signbit(got[0, 0, 0, 1]) and not np.signbit(got[0, 0, 0, 0]) and not np.signbit(got[0, 0, 2, 2])
    for case in bc.EVEN_CASES:
        _, want = bc.even_want(case)
        assert np.signbit(want[0, 0, 1, 1]) and want[0, 0, 1, 1] == 0, case


def test_the_weight_gradient_is_conv2ds():
    for case in (bc.WGRAD[8], bc.WGRAD[12], bc.WGRAD[-3], bc.WGRAD[-2]):
        layer, x, g = bc.wgrad_data(case)
        k, stride = case[1], case[2]
        w = t64(layer['weight']).requires_grad_()
        b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
        out = F.conv2d(t64(x), w, b, stride, k // 2)
        if layer['scale'] is not None:
            out = out * t64(layer['scale']).reshape(1, -1, 1, 1)
        out.backward(t64(g))
        wg = bc.wgrad_want(case)
        close(case[0] + ' dW', wg['dW'], w.grad.numpy(), 1e-13)
        if layer['scale'] is None:
            close(case[0] + ' db', wg['db'], b.grad.numpy(), 1e-13)
        else:
            assert wg['db'] is None


def test_ws_is_rounded_once():
    layer = bc.dgrad_data(bc.DGRAD[0])[0]
    ws = ref.ws_of(layer)
    exact = layer['weight'].astype(np.float64) * layer['scale'].astype(np.float64)[:, None, None, None]
    assert ws.dtype == F32 and np.array_equal(ws, exact.astype(F32))
    assert np.abs(ws - exact).max() > 0                                           # the product is inexact: the rounding is there to be counted
    assert ref.ws_of(dict(layer, scale=None)) is not None and np.array_equal(ref.ws_of(dict(layer, scale=None)), layer['weight'])
    # the packing holds ws transposed with its taps flipped: element [nt][tap][kb][lane][e] = ws[16 kb + 4 (lane >> 4) + e][:, 8 - tap][16 nt + (lane & 15)]
    p = ref.pack_bwd(layer).reshape(-1, 9, 2, 4, 16, 4)
    assert p[1, 2, 1, 1, 3, 2] == ws[16 + 4 + 2, 16 + 3, 2, 0] and p[0, 0, 0, 0, 0, 0] == ws[0, 0, 2, 2]


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------------
def test_the_trainable_trunk_refuses_before_it_touches_a_device():
    from cosypose_amd import Detector, DetectorTrunk
    sd = bc.torch_sd()
    with pytest.raises(ValueError, match='float32 only'):
        DetectorTrunk.from_state_dict(sd, dtype=torch.float16, device='cuda', trainable=True)
    with pytest.raises(ValueError, match='stem'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=0)
    with pytest.raises(ValueError, match='exceeds'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=bc.N_STAGES + 2)
    with pytest.raises(ValueError, match='train_from_stage must be an int'):
        DetectorTrunk.from_state_dict(sd, device='cuda', trainable=True, train_from_stage=2.0)
    with pytest.raises(ValueError, match='ROCm device'):
        DetectorTrunk.from_state_dict(sd, trainable=True)
    with pytest.raises(KeyError, match='backbone.body.conv1.weight'):
        DetectorTrunk.from_state_dict({k: v for k, v in sd.items() if k != 'backbone.body.conv1.weight'}, device='cuda', trainable=True)
    with pytest.raises(KeyError, match='backbone.body.layer1.0.conv1.weight'):
        DetectorTrunk.from_state_dict({k: v for k, v in sd.items() if '.body.layer' not in k}, device='cuda', trainable=True)
    with pytest.raises(ValueError, match='float32 only'):
        Detector.from_state_dict(sd, tc.E2E_LABELS, dtype=torch.bfloat16, trainable=True)
    plain = DetectorTrunk.from_state_dict(sd)
    for what in ('parameters', 'named_parameters', 'state_dict'):
        with pytest.raises(RuntimeError, match='trainable=True'):
            getattr(plain, what)()
    with pytest.raises(RuntimeError, match='trainable=True'):
        plain.pack_count


def test_the_new_exports_are_bound_with_the_headers_arity():
    import cosypose_amd
    from cosypose_amd import _lib
    want = {'cosy_trunk_weight_pack': 10, 'cosy_trunk_dgrad': 12, 'cosy_trunk_wgrad': 9}
    for name, n in want.items():
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][0]) == n and _lib._SIGNATURES[name][1] is _lib._I, name
    assert (_lib.TRUNK_ADD_NONE, _lib.TRUNK_ADD_SAME, _lib.TRUNK_ADD_EVEN, _lib.TRUNK_ADD_NEAREST_T) == (0, 1, 2, 3)
    for name in ('TrainableTrunkLayer', 'trunk_dgrad', 'trunk_wgrad', 'layer_dgrad', 'layer_wgrad', 'DetectorTrunk', 'Detector'):
        assert getattr(cosypose_amd, name) is not None

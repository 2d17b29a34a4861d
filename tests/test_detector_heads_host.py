"""CPU tests of the detector's heads: the twin tests/dethead_ref.py against torch's own float64 layers, the head
structures against the twin's chaining, the weight packing, the C ABI's declarations and the Python layer's argument checks.  No GPU."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import dethead_case as case
import dethead_ref as ref
from cosypose_amd import detector_heads
from cosypose_amd.detector_heads import DetectorHeads, HeadLayer, conv_layer

REPO = pathlib.Path(__file__).resolve().parent.parent
HEAD_SYMBOLS = ('cosy_head_big_rows', 'cosy_head_max_tile_rows', 'cosy_head_pack', 'cosy_head_conv')


def torch64(layer, x):
    w, b, x = (torch.from_numpy(np.asarray(v, np.float64)) for v in (layer['weight'], layer['bias'], x))
    if layer['kind'] == 'linear':
        y = Fn.linear(x, w, b)
    elif layer['kind'] == 'deconv':
        y = Fn.conv_transpose2d(x, w, b, stride=2)
    else:
        y = Fn.conv2d(x, w, b, padding=w.shape[2] // 2)
    return (torch.relu(y) if layer['relu'] else y).numpy()


@pytest.mark.parametrize('c', case.CASES, ids=case.case_id)
def test_the_twins_float64_layers_equal_torchs(c):
    layer, x = case.case_data(c)
    got, S, K = ref.layer64(layer, x)
    want = torch64(layer, x)
    assert got.shape == want.shape and K == {'conv3': 9, 'conv1': 1, 'linear': 1, 'deconv': 1}[c[0]] * c[1]
    assert (np.abs(got - want) <= 1e-12 * S).all()
    assert (S >= np.abs(want)).all()


@pytest.mark.parametrize('c', case.CASES, ids=case.case_id)
def test_the_float32_chain_is_safe_on_the_chosen_seeds_and_within_the_bound(c):
    got = case.want32(c)                                            # raises DoubleRounding where the emulation cannot promise fmaf's bits
    want, bound = case.want64(c, 'float32')
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= bound).all()


def test_storage_rounding_is_torchs():
    x = np.concatenate([np.random.RandomState(0).normal(0, 1, 4096) * 10.0 ** np.random.RandomState(1).randint(-9, 5, 4096), [0.0, -0.0, 65520.0, 1e-8, 3e38]])
    for name, dt in (('float16', torch.float16), ('bfloat16', torch.bfloat16)):
        want = torch.from_numpy(x.astype(np.float32)).to(dt).double().numpy()
        assert np.array_equal(ref.round_to(x, name), want)
    assert ref.storage_ulp(np.array([1.0, 1.5, 2.0, 2.0 ** -20]), 'float16').tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24]
    assert ref.storage_ulp(np.array([1.0, 3.0, 0.25]), 'bfloat16').tolist() == [2.0 ** -7, 2.0 ** -6, 2.0 ** -9]


def test_the_head_structures_equal_the_twins_chaining():
    sd, (feats, roi, mroi) = case.head_weights(), case.head_inputs()
    rpn, box_head, box_pred, mask_head, mask_pred = case.torch_heads(dtype=torch.float64)
    want = case.head_wants('float32')                               # float32 weights, no storage rounding: the float64 value of the modules
    obj, dl = rpn([torch.from_numpy(f).double() for f in feats])
    for l in range(len(feats)):
        v_o, e_o, v_d, e_d = want['rpn'][l]
        assert np.abs(obj[l].numpy() - v_o).max() <= 1e-12 and np.abs(dl[l].numpy() - v_d).max() <= 1e-12
        assert e_o.shape == v_o.shape and (e_o > 0).all() and e_o.max() < 1e-3
    cls, reg = box_pred(box_head(torch.from_numpy(roi).double()))
    assert np.abs(cls.numpy() - want['box'][0]).max() <= 1e-12 and np.abs(reg.numpy() - want['box'][2]).max() <= 1e-12
    m = mask_pred(mask_head(torch.from_numpy(mroi).double())).numpy()
    assert m.shape == (3, case.K, 28, 28) and np.abs(m - want['mask'][0]).max() <= 1e-12
    # the running bound grows with a 16-bit storage type, output by output
    assert (case.head_wants('float16')['mask'][1] > want['mask'][1]).all() and (case.head_wants('float16')['box'][1] > want['box'][1]).all()
    assert sd['rpn.head.conv.weight'].dtype == np.float32


def tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_from_state_dict_and_from_modules_pack_the_same_bytes(dtype):
    sd = tensors(case.head_weights())
    a = DetectorHeads.from_state_dict(sd, dtype=dtype)
    b = DetectorHeads.from_modules(*case.torch_heads(), dtype=dtype)
    assert len(a.layers()) == len(b.layers()) == 11
    for la, lb in zip(a.layers(), b.layers()):
        assert la.packed.dtype == dtype and la.packed.shape == lb.packed.shape
        assert la.packed.view(torch.uint8).equal(lb.packed.view(torch.uint8)) and la.packed_bias.equal(lb.packed_bias)
        assert (la.kind, la.ksize, la.c_in, la.c_out, la.relu) == (lb.kind, lb.ksize, lb.c_in, lb.c_out, lb.relu)
    assert a.rpn_head.A == case.A and a.box_head.K == case.K and a.mask_head.logits.c_out == case.K
    no_mask = DetectorHeads.from_modules(*case.torch_heads()[:3], dtype=dtype)
    assert no_mask.mask_head is None and len(no_mask.layers()) == 5


def test_packing_puts_every_weight_where_the_header_says():
    rng = np.random.RandomState(2)
    w = torch.from_numpy(rng.normal(0, 1, (19, 9, 40)).astype(np.float32))
    for dtype, KB in ((torch.float32, 16), (torch.float16, 32), (torch.bfloat16, 32)):
        E, KBn = KB // 4, -(-40 // KB)
        p = detector_heads.pack_weight(w, dtype).float().view(4, 9, KBn, 64, E)
        ref_w = w.to(dtype).float()
        for nt, tap, kb, lane, e in [(0, 0, 0, 0, 0), (1, 4, 1, 37, 3), (1, 8, KBn - 1, 63, E - 1), (3, 2, 0, 5, 1), (0, 5, 2 if KB == 16 else 1, 17, 1)]:
            k = KB * kb + E * (lane >> 4) + e
            n = 16 * nt + (lane & 15)
            want = float(ref_w[n, tap, k]) if n < 19 and k < 40 else 0.0
            assert float(p[nt, tap, kb, lane, e]) == want, (dtype, nt, tap, kb, lane, e)


def test_a_missing_head_key_is_a_key_error_that_names_it():
    sd = tensors(case.head_weights())
    for key in ('rpn.head.bbox_pred.bias', 'roi_heads.box_head.fc7.weight', 'roi_heads.mask_predictor.conv5_mask.weight'):
        with pytest.raises(KeyError, match=re.escape(key)):
            DetectorHeads.from_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match='go together'):
        DetectorHeads.from_modules(*case.torch_heads()[:4])


def test_c_abi_declares_exports_and_builds_the_head_entry_points():
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES, FLAGS
    build()
    for name in HEAD_SYMBOLS:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_dethead.hip' in SOURCES and '-packed-fp32-ops' in FLAGS
    src = (REPO / 'cosypose_amd' / 'csrc' / 'kernels_dethead.hip').read_text()
    assert int(re.search(r'constexpr int HEAD_BIG_ROWS = (\d+);', src).group(1)) == case.BIG_ROWS          # the tests size their cases by these
    assert 64 * int(re.search(r'constexpr int HEAD_MT_BIG = (\d+)', src).group(1)) == case.TILE_ROWS
    assert not re.search(r'atomic[A-Z_(]', src) and 'fmaxf' not in src       # no floating-point atomics; ReLU keeps a NaN


def test_argument_checks_of_the_python_layer():
    heads = DetectorHeads.from_state_dict(tensors(case.head_weights()))
    feats, roi, mroi = case.head_inputs()
    t = torch.from_numpy
    with pytest.raises(ValueError, match='ROCm device'):
        heads.rpn_head([t(f) for f in feats])
    with pytest.raises(ValueError, match='ROCm device'):
        heads.box_head(t(roi))
    with pytest.raises(ValueError, match='ROCm device'):
        heads.mask_head(t(mroi))
    with pytest.raises(ValueError, match='list of one tensor per level'):
        heads.rpn_head(t(feats[0]))
    with pytest.raises(ValueError, match='1 to 8 levels'):
        heads.rpn_head([])
    with pytest.raises(ValueError, match=r'features\[1\] must be torch.float32'):
        heads.rpn_head([t(feats[0]), t(feats[1]).double()])
    with pytest.raises(ValueError, match=r'features\[0\] must be \(B,C,H,W\) with 16 channels'):
        heads.rpn_head([t(feats[0])[:, :8]])
    with pytest.raises(ValueError, match='392 channels'):
        heads.box_head(t(roi)[:, :, :6])
    with pytest.raises(ValueError, match=r'roi_feats must be \(R,C,P,P\)'):
        heads.box_head(t(roi)[0])
    with pytest.raises(ValueError, match='must be torch.float32'):
        heads.mask_head(t(mroi).half())
    with pytest.raises(ValueError, match='16 channels'):
        heads.mask_head(t(mroi)[:, :8])
    with pytest.raises(ValueError, match='must be a HeadLayer'):
        conv_layer(t(mroi), None)
    with pytest.raises(ValueError, match='dtype must be'):
        DetectorHeads.from_state_dict(tensors(case.head_weights()), dtype=torch.float64)
    with pytest.raises(ValueError, match='multiple of 8'):
        HeadLayer.conv(torch.zeros(4, 12, 3, 3))
    with pytest.raises(ValueError, match='3x3 or 1x1'):
        HeadLayer.conv(torch.zeros(4, 8, 5, 5))
    with pytest.raises(ValueError, match=r'ConvTranspose2d\(k=2, s=2\)'):
        HeadLayer.deconv(torch.zeros(8, 8, 3, 3))
    sd = dict(tensors(case.head_weights()))
    sd['rpn.head.bbox_pred.weight'] = sd['rpn.head.bbox_pred.weight'][:8]
    sd['rpn.head.bbox_pred.bias'] = sd['rpn.head.bbox_pred.bias'][:8]
    with pytest.raises(ValueError, match='4 x the 3 outputs'):
        DetectorHeads.from_state_dict(sd)
    import cosypose_amd
    assert cosypose_amd.DetectorHeads is DetectorHeads and cosypose_amd.conv_layer is conv_layer and cosypose_amd.HeadLayer is HeadLayer

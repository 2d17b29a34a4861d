"""The CPU twin of the detector's trunk (tests/dettrunk_ref.py) against torch's own float64 layers, and everything of
cosypose_amd/detector_trunk.py that needs no device: the loader, the packed bytes, the refusals, the header."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dettrunk_case as case
import dettrunk_ref as ref
from frames_ref import DoubleRounding

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'cosyhip.h')


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def torch_layer(layer, x, r=None):
    w = t64(layer['weight'])
    y = F.conv2d(t64(x), w, None, layer['stride'], w.shape[2] // 2)
    if layer['scale'] is not None:
        y = y * t64(layer['scale']).reshape(1, -1, 1, 1)
    y = y + t64(layer['bias']).reshape(1, -1, 1, 1)
    if r is not None:
        y = y + F.interpolate(t64(r), size=y.shape[-2:], mode='nearest')
    return (torch.relu(y) if layer['relu'] else y).numpy()


@pytest.mark.parametrize('c', case.CASES, ids=case.case_id)
def test_the_twins_layers_equal_torchs_float64_layers(c):
    layer, x, r = case.case_data(c)
    got, A, K = ref.layer64(layer, x, r)
    want = torch_layer(layer, x, r)
    assert got.shape == want.shape and rel(got, want) <= 1e-12
    assert K == layer['weight'].shape[1] * layer['weight'].shape[2] ** 2 and (A >= np.abs(got)).all()


def test_the_fmaf_chains_stay_clear_of_double_rounding_and_within_the_bound():
    """SALT's purpose: no case may trip frames_ref.fma32's guard; and the chain itself obeys the bound it is the reference of"""
    try:
        for c in case.CASES:
            want, bound = case.want64(c, 'float32')
            assert (np.abs(case.want32(c).astype(np.float64) - want) <= bound).all(), case.case_id(c)
        for shape in case.STEMS:
            layer, _, _, _, images = case.stem_data(shape)
            ref.layer32(layer, ref.stem_columns(images))
    except DoubleRounding as e:           # pragma: no cover
        pytest.fail(f'choose another SALT: {e}')


@pytest.mark.parametrize('shape', case.STEMS, ids=str)
def test_the_stem_columns_are_the_7x7_stride_2_convolution(shape):
    layer, w, scale, shift, images = case.stem_data(shape)
    cols = ref.stem_columns(images)
    assert cols.shape[1] == 152 and (cols[:, 147:] == 0).all() and not np.signbit(cols[:, 147:]).any()
    got = ref.layer64(layer, cols)[0]
    y = F.conv2d(t64(images), t64(w), None, 2, 3) * t64(scale).reshape(1, -1, 1, 1) + t64(shift).reshape(1, -1, 1, 1)
    assert rel(got, torch.relu(y).numpy()) <= 1e-12


@pytest.mark.parametrize('shape', case.POOLS, ids=str)
def test_the_pool_pads_with_minus_infinity_and_takes_a_nan_as_torch_does(shape):
    x = case.pool_data(shape)
    assert (x[~np.isnan(x)] < 0).all() and int(np.isnan(x).sum()) == 1
    got, want = ref.maxpool(x), F.max_pool2d(torch.from_numpy(x), 3, 2, 1).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]) and (got[~np.isnan(got)] < 0).all()
    for dtype in case.DTYPES:
        assert np.array_equal(np.nan_to_num(ref.ref.round_to(x, dtype)), np.nan_to_num(x.astype(np.float64)))      # exact in every storage type


def test_the_nearest_rule_equals_interpolate_for_every_small_size():
    for n_in in range(1, 65):
        for n_out in (2 * n_in - 1, 2 * n_in):
            src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
            want = F.interpolate(src, size=(n_out, 1), mode='nearest').reshape(-1).long().numpy()
            assert np.array_equal(ref.nearest_index(n_in, n_out), want), (n_in, n_out)


@pytest.fixture(scope='module')
def emulated():
    return case.trunk_emulated(case.INPUTS[1], 'float32')


def test_the_twins_bottlenecks_and_fpn_equal_torch_in_float64(emulated):
    """the twin's float32-weight chain in float64 (float32 stores nothing it would round) against the torch.nn restatement of the network, block by
    block and through the FPN with its non-integer top-down ratio (23 x 39 -> 12 x 20 -> 6 x 10 -> 3 x 5)"""
    net, m = case.trunk_net(), case.torch_trunk().double()
    (maps, keep) = emulated
    for (s, i), x in [(k, v) for k, v in keep.items() if k != 'feats']:
        got = ref.bottleneck(net['stages'][s - 1][i], x, None, 'float32')[0]
        want = getattr(m.body, f'layer{s}')[i](t64(x)).numpy()
        assert rel(got, want) <= 1e-12, (s, i)
    feats = keep['feats']
    assert [f.shape[2:] for f in feats] == [(12, 20), (6, 10), (3, 5), (2, 3)]
    got = ref.fpn(net, [(f, None) for f in feats], 'float32')
    want = m.fpn([t64(f) for f in feats])
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert g[0].shape == tuple(w.shape) and rel(g[0], w.numpy()) <= 1e-12


def test_the_twins_whole_trunk_equals_torch_in_float64(emulated):
    maps, _ = emulated
    want = case.torch_trunk().double()(t64(ref.ref.round_to(case.trunk_images(case.INPUTS[1]), 'float32')))
    for (v, e), w in zip(maps, want):
        assert v.shape == tuple(w.shape) and rel(v, w.numpy()) <= 1e-11          # 53 layers of float64 roundings in two orders
        assert (e >= 0).all() and np.isfinite(e).all()


# ---- the loader ----------------------------------------------------------------------------------------------------------------------------
def sd_torch(sd=None):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in (case.trunk_weights() if sd is None else sd).items()}


def test_from_state_dict_and_from_modules_pack_equal_bytes_and_the_twins_scale_and_shift():
    from cosypose_amd import DetectorTrunk
    a = DetectorTrunk.from_state_dict(sd_torch())
    b = DetectorTrunk.from_modules(case.torch_trunk())
    assert [len(s) for s in a.stages] == list(case.BLOCKS) and len(a.layers()) == len(b.layers()) == 1 + 3 * 16 + 4 + 8
    for x, y in zip(a.layers(), b.layers()):
        assert x.packed.numpy().tobytes() == y.packed.numpy().tobytes() and x.packed_bias.numpy().tobytes() == y.packed_bias.numpy().tobytes()
        assert (x.packed_scale is None) == (y.packed_scale is None)
        assert x.packed_scale is None or x.packed_scale.numpy().tobytes() == y.packed_scale.numpy().tobytes()
        assert (x.stride, x.ksize, x.relu, x.c_in, x.c_out) == (y.stride, y.ksize, y.relu, y.c_in, y.c_out)
    net = case.trunk_net()
    twin = [net['stem']] + [blk[k] for blocks in net['stages'] for blk in blocks for k in ('conv1', 'conv2', 'conv3', 'down') if blk[k] is not None]
    twin += net['inner'] + net['outer']
    for x, t in zip(a.layers(), twin):                       # scale and shift in float32, the twin's bits; stride and ReLU where the twin has them
        n = x.c_out
        assert np.array_equal(x.packed_bias.numpy()[:n].view(np.int32), np.asarray(t['bias'], np.float32).view(np.int32)), x.name
        assert (x.packed_scale is None) == (t['scale'] is None)
        if t['scale'] is not None:
            assert np.array_equal(x.packed_scale.numpy()[:n].view(np.int32), t['scale'].view(np.int32)), x.name
        assert (x.stride, x.relu) == (t['stride'], t['relu']), x.name
    half = DetectorTrunk.from_state_dict(sd_torch(), dtype=torch.float16)
    assert half.stem.packed.dtype == torch.float16 and half.stem.packed_scale.dtype == torch.float32


def test_a_missing_key_is_a_key_error_that_names_it():
    from cosypose_amd import DetectorTrunk
    for key in ('backbone.body.layer3.4.bn2.running_var', 'backbone.fpn.layer_blocks.2.bias', 'backbone.body.conv1.weight',
                'backbone.body.layer2.0.downsample.1.weight'):
        sd = sd_torch()
        del sd[key]
        with pytest.raises(KeyError, match=re.escape(key)):
            DetectorTrunk.from_state_dict(sd)


def test_an_odd_width_is_a_value_error_that_names_the_layer():
    from cosypose_amd import DetectorTrunk
    sd = sd_torch()
    sd['backbone.body.layer1.1.conv1.weight'] = torch.zeros(12, 32, 1, 1)
    with pytest.raises(ValueError, match=re.escape('backbone.body.layer1.1.conv1')):
        DetectorTrunk.from_state_dict(sd)
    with pytest.raises(ValueError, match='float32, torch.float16 or torch.bfloat16'):
        DetectorTrunk.from_state_dict(sd_torch(), dtype=torch.float64)


def test_keys_that_are_not_the_trunks_are_ignored():
    from cosypose_amd import DetectorTrunk
    sd = sd_torch()
    assert 'backbone.body.bn1.num_batches_tracked' in sd and 'rpn.head.conv.bias' in sd
    a = DetectorTrunk.from_state_dict(sd)
    b = DetectorTrunk.from_state_dict({k: v for k, v in sd.items() if 'num_batches_tracked' not in k and k.startswith('backbone.')})
    assert all(x.packed.numpy().tobytes() == y.packed.numpy().tobytes() for x, y in zip(a.layers(), b.layers()))


def test_cpu_tensors_and_wrong_channel_counts_are_refused_before_the_device():
    from cosypose_amd import DetectorTrunk
    trunk = DetectorTrunk.from_state_dict(sd_torch())
    with pytest.raises(ValueError, match='ROCm device'):
        trunk(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match='channels'):
        trunk(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match='stage outputs'):
        trunk.fpn([torch.zeros(1, 8, 2, 2)] * 5)


# ---- the header ----------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_and_exported():
    from cosypose_amd import _lib
    for name in ('cosy_trunk_conv', 'cosy_trunk_stem_pack', 'cosy_trunk_maxpool'):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).restype is _lib._I
    assert len(_lib._SIGNATURES['cosy_trunk_conv'][0]) == 7 and _lib._SIGNATURES['cosy_trunk_conv'][0][1] is _lib._I


def test_the_header_gained_no_struct():
    import test_c_abi
    text = open(HEADER).read()
    structs = set(re.findall(r'}\s*(cosy_\w+_t)\s*;', text))
    listed = open(test_c_abi.__file__).read()
    assert structs and all(s in listed for s in structs)
    assert 'cosy_trunk' not in ' '.join(structs)

"""The detector's trunk on the GPU (csrc/kernels_dettrunk.hip behind cosypose_amd/detector_trunk.py) against the CPU twin tests/dettrunk_ref.py,
which test_detector_trunk_host.py holds against torch's own float64 layers.

Criterion of a single layer: |got - want| <= (K + 3) u (|scale| S + |shift| + |residual|) per output against the twin's float64 evaluation fed the
operands rounded to the type, S = sum |w x|, u = 2^-24 for float32 and 2^-23 for the 16-bit types: K roundings of the chain (section 26), one of
the fused scale / shift, one of the residual add; a ROWS store in a 16-bit type rounds the result once more, half an ulp of that type (with_store).
float32 also: BIT-equal to the twin's fmaf chain.  Pool and stem pack: exact.
The whole trunk on the narrow net: float32 bit-equal to the chained chains; 16-bit per bottleneck and through the FPN within the twin's running
bound; 16-bit whole trunk within 2 x the difference the twin itself shows between rounding every stored intermediate and rounding none.
Every test prints its largest error as a share of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import dettrunk_case as case
import dettrunk_ref as ref
from cosypose_amd import DetectorTrunk, TrunkLayer, trunk_conv_layer
from cosypose_amd import _lib
from cosypose_amd import detector_trunk as dt

pytestmark = pytest.mark.gpu
TORCH = {'float32': torch.float32, 'float16': torch.float16, 'bfloat16': torch.bfloat16}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest share of the bound = {share:.3f}')
    return err


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def with_store(c, dtype, want, bound):
    """the bound of section 27 holds for the value the epilogue hands to the store.  A NCHW store is float32 and adds nothing; a ROWS store in a
    16-bit type rounds that value once more, to nearest: half a unit in the last place of the type at |want| + bound, added here"""
    if c[5] == 'rows' and dtype != 'float32':
        return bound + ref.ref.storage_ulp(np.abs(want) + bound, dtype) / 2
    return bound


def trunk_layer(layer, dtype, name='case'):
    bn = None
    if layer['scale'] is not None:                     # scale = weight * rsqrt(1), shift = bias - 0 * scale: the twin's scale and shift to the bit
        bn = (torch.from_numpy(layer['scale']), torch.from_numpy(layer['bias']), torch.zeros(len(layer['bias'])), torch.ones(len(layer['bias'])))
    return TrunkLayer(name, torch.from_numpy(layer['weight']), bn=bn, bias=None if bn else torch.from_numpy(layer['bias']), stride=layer['stride'],
                      relu=layer['relu'], dtype=TORCH[dtype], device='cuda')


def run_case(c, dtype, x=None):
    layer, x0, r = case.case_data(c)
    x = x0 if x is None else x
    got = trunk_conv_layer(dev(x), trunk_layer(layer, dtype), None if r is None else dev(r), store=c[5])
    if c[5] == 'rows':
        B, H, W = c[6]
        Ho, Wo = ref.out_size(H, c[2]), ref.out_size(W, c[2])
        assert got.dtype == TORCH[dtype] and tuple(got.shape) == (B * Ho * Wo, c[4])
        got = got.view(B, Ho, Wo, c[4]).permute(0, 3, 1, 2).float()
    assert got.dtype == torch.float32
    return got.cpu().numpy()


@pytest.fixture(scope='module')
def trunks():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in case.trunk_weights().items()}
    return {d: DetectorTrunk.from_state_dict(sd, dtype=TORCH[d], device='cuda') for d in case.DTYPES}


# ---- single layers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', case.DTYPES)
@pytest.mark.parametrize('c', case.CASES, ids=case.case_id)
def test_a_layer_meets_the_float64_bound_and_in_float32_the_chains_bits(c, dtype):
    want, bound = case.want64(c, dtype)
    got = run_case(c, dtype)
    assert got.shape == want.shape
    bound = with_store(c, dtype, want, bound)
    err = report(f'{case.case_id(c)} {dtype}', got, want, bound)
    assert (err <= bound).all()
    if dtype == 'float32':
        differ = int((bits(got) != bits(case.want32(c))).sum())
        print(f'  outputs whose bits differ from the fmaf chain: {differ} of {got.size}')
        assert differ == 0


@pytest.mark.parametrize('dtype', case.DTYPES)
@pytest.mark.parametrize('shape', case.STEMS, ids=str)
def test_the_stem_pack_is_exact_and_the_stem_meets_the_bound(shape, dtype):
    layer, w, scale, shift, images = case.stem_data(shape)
    B, _, H, W = shape
    Ho, Wo = ref.out_size(H, 2), ref.out_size(W, 2)
    rows = torch.full((B * Ho * Wo, 152), 7.0, dtype=TORCH[dtype], device='cuda')
    assert _lib.lib().cosy_trunk_stem_pack(_lib.ptr(dev(images)), _lib.ptr(rows), B, H, W, _lib.DTYPES[TORCH[dtype]], _lib.stream()) == 0
    cols = ref.ref.round_to(ref.stem_columns(images), dtype)
    got = rows.view(B, Ho, Wo, 152).permute(0, 3, 1, 2).double().cpu().numpy()
    assert np.array_equal(got, cols) and not np.signbit(got[:, 147:]).any()
    tl = TrunkLayer('stem', torch.from_numpy(w), bn=(torch.from_numpy(scale), torch.from_numpy(shift), torch.zeros(8), torch.ones(8)), stride=2, relu=True,
                    dtype=TORCH[dtype], device='cuda')
    out = trunk_conv_layer(dev(images), tl).cpu().numpy()
    want, A, K = ref.layer64(layer, ref.stem_columns(images), None, dtype)
    assert K == 152
    bound = (K + 3) * ref.U[dtype] * A
    assert (report(f'stem {shape} {dtype}', out, want, bound) <= bound).all()
    if dtype == 'float32':
        assert np.array_equal(bits(out), bits(ref.layer32(layer, ref.stem_columns(images))))


@pytest.mark.parametrize('dtype', case.DTYPES)
@pytest.mark.parametrize('shape', case.POOLS, ids=str)
def test_the_pool_is_exact_pads_with_minus_infinity_and_takes_a_nan(shape, dtype):
    x = case.pool_data(shape)
    want = ref.maxpool(x)
    got = dt.max_pool(dev(x), TORCH[dtype]).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]) and (got[ok] < 0).all()


@pytest.mark.parametrize('dtype', case.DTYPES)
def test_a_nan_reaches_exactly_its_receptive_field_and_relu_keeps_it(dtype):
    for c, where in ((case.STRIDED[16], (1, 7, 2, 3)), (case.STRIDED[0], (0, 3, 4, 6)), (case.RESIDUAL[0], (1, 7, 2, 3))):
        layer, x, r = case.case_data(c)
        assert layer['relu']
        x = x.copy()
        x[where] = np.nan
        want, A, K = ref.layer64(layer, x, r, dtype)
        got = run_case(c, dtype, x)
        assert 0 < int(np.isnan(want).sum()) < want.size and np.array_equal(np.isnan(got), np.isnan(want)), case.case_id(c)
        ok = ~np.isnan(want)
        with np.errstate(invalid='ignore'):
            bound = with_store(c, dtype, np.nan_to_num(want), np.nan_to_num((K + 3) * ref.U[dtype] * A))
        assert (report(f'{case.case_id(c)} {dtype} beside a NaN', got[ok], want[ok], bound[ok]) <= bound[ok]).all()


def test_two_calls_give_equal_bits_and_an_empty_batch_is_served():
    for c in (case.STRIDED[16], case.RESIDUAL[1], case.BIG[1]):
        a, b = run_case(c, 'float16'), run_case(c, 'float16')
        assert np.array_equal(bits(a), bits(b))
    layer, x, r = case.case_data(case.RESIDUAL[1])
    tl = trunk_layer(layer, 'float32')
    none = trunk_conv_layer(dev(x[:0]), tl, dev(r[:0]))
    assert tuple(none.shape) == (0, 24, 5, 7) and none.is_cuda and none.dtype == torch.float32
    assert tuple(dt.max_pool(dev(case.pool_data(case.POOLS[0])[:0])).shape) == (0, 8, 3, 4)
    stem = case.stem_data(case.STEMS[0])
    tl = TrunkLayer('stem', torch.from_numpy(stem[1]), bias=torch.zeros(8), stride=2, device='cuda')
    assert tuple(trunk_conv_layer(dev(stem[4][:0]), tl).shape) == (0, 8, 5, 6)


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------------------
def test_c_abi_trunk_refusals():
    l_ = _lib.lib()
    c = case.STRIDED[20]                               # k 3, stride 2, 40 -> 15 channels as NCHW on (5, 7)
    assert c[1] == 3 and c[5] == 'nchw'
    layer, x, _ = case.case_data(c)
    B, H, W = c[6]
    Ho, Wo = ref.out_size(H, 2), ref.out_size(W, 2)
    tl = trunk_layer(layer, 'float32')
    rows = dt._to_rows(dev(x), torch.float32)
    res = torch.zeros((B * Ho * Wo, 16), device='cuda')
    out = torch.full((B, c[4], Ho, Wo), -777.0, device='cuda')

    def call(stride=2, scale=True, residual=None, res_hw=(0, 0), **change):
        d = _lib.HeadLayer()
        d.x, d.w, d.bias, d.out, d.out1 = _lib.ptr(rows), _lib.ptr(tl.w), _lib.ptr(tl.bias), _lib.ptr(out), None
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_F32, 3, c[3], c[4], 1, _lib.HEAD_STORE_NCHW, c[4], 1
        d.row_start[0], d.row_start[1], d.H[0], d.W[0] = 0, B * H * W, H, W
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return l_.cosy_trunk_conv(ctypes.byref(d), stride, _lib.ptr(tl.scale) if scale else None, residual, res_hw[0], res_hw[1], _lib.stream())
    bad = [dict(stride=0), dict(stride=3), dict(dtype=3), dict(ksize=2), dict(ksize=7), dict(c_in=12), dict(c_in=0), dict(c_out=0), dict(relu=2),
           dict(store=_lib.HEAD_STORE_DECONV_ROWS), dict(store=_lib.HEAD_STORE_DECONV_NCHW), dict(store=4), dict(store=-1), dict(n_split=3),
           dict(store=_lib.HEAD_STORE_ROWS), dict(n_levels=0), dict(n_levels=9), dict(n_levels=2, row_start=(2, B * H * W), H=(1, H), W=(1, W)),
           dict(stride=1, n_levels=2, row_start=(2, B * H * W), H=(1, H), W=(1, W), residual=res.data_ptr(), res_hw=(Ho, Wo), c_out=16, n_split=16),
           dict(row_start=(0, 1)), dict(row_start=(1, B * H * W - 1)), dict(H=(0, 0)), dict(W=(0, 0)), dict(x=None), dict(w=None), dict(bias=None),
           dict(out=None), dict(x=rows.data_ptr() + 4), dict(residual=res.data_ptr(), res_hw=(Ho, Wo)), dict(residual=res.data_ptr(), res_hw=(0, 1), c_out=16, n_split=16),
           dict(residual=res.data_ptr() + 4, res_hw=(Ho, Wo), c_out=16, n_split=16)]
    for change in bad:
        assert call(**change) == -1, change
        assert l_.cosy_last_error().decode().startswith('cosy_trunk_conv:'), (change, l_.cosy_last_error())
    assert l_.cosy_trunk_conv(None, 2, None, None, 0, 0, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (out == -777.0).all()                                    # no refused call launched anything
    assert call(row_start=(1, 0), x=None, w=None, bias=None, out=None) == 0       # M = 0: success, nothing launched, null pointers allowed
    img = dev(case.stem_data(case.STEMS[0])[4])
    cols = torch.empty((2 * 5 * 6, 152), device='cuda')
    for args in ((None, _lib.ptr(cols), 2, 9, 11, 0), (_lib.ptr(img), None, 2, 9, 11, 0), (_lib.ptr(img), _lib.ptr(cols), -1, 9, 11, 0),
                 (_lib.ptr(img), _lib.ptr(cols), 2, 0, 11, 0), (_lib.ptr(img), _lib.ptr(cols), 2, 9, 11, 5), (_lib.ptr(img), cols.data_ptr() + 4, 2, 9, 11, 0)):
        assert l_.cosy_trunk_stem_pack(*args, _lib.stream()) == -1, args
        assert l_.cosy_last_error().decode().startswith('cosy_trunk_stem_pack:')
    assert l_.cosy_trunk_stem_pack(None, None, 0, 9, 11, 0, _lib.stream()) == 0
    for args in ((None, _lib.ptr(cols), 1, 5, 7, 8, 0), (_lib.ptr(cols), None, 1, 5, 7, 8, 0), (_lib.ptr(cols), _lib.ptr(res), 1, 5, 7, 12, 0),
                 (_lib.ptr(cols), _lib.ptr(res), 1, 5, 7, 0, 0), (_lib.ptr(cols), _lib.ptr(res), 1, 0, 7, 8, 0), (_lib.ptr(cols), _lib.ptr(res), -1, 5, 7, 8, 0),
                 (_lib.ptr(cols), _lib.ptr(res), 1, 5, 7, 8, 3)):
        assert l_.cosy_trunk_maxpool(*args, _lib.stream()) == -1, args
        assert l_.cosy_last_error().decode().startswith('cosy_trunk_maxpool:')
    assert l_.cosy_trunk_maxpool(None, None, 0, 5, 7, 8, 0, _lib.stream()) == 0
    assert call() == 0
    want, bound = case.want64(c, 'float32')
    assert (np.abs(out.cpu().numpy() - want) <= bound).all()


# ---- the whole trunk on the narrow net ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', case.INPUTS, ids=str)
def test_the_float32_trunk_holds_the_bits_of_the_chained_fmaf_chains(trunks, shape):
    want, _ = case.trunk_bits(shape)
    x = dev(case.trunk_images(shape))
    with torch.no_grad():
        got = trunks['float32'](x)
        again = trunks['float32'](x)
    assert len(got) == len(want) == 5
    for name, g, a, w in zip(dt.LEVELS, got, again, want):
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32 and g.is_contiguous()
        differ = int((bits(g.cpu().numpy()) != bits(w)).sum())
        print(f'level {name} {tuple(g.shape)}: outputs whose bits differ from the chained chains: {differ} of {w.size}')
        assert differ == 0
        assert g.data_ptr() != a.data_ptr() and torch.equal(g.view(torch.int32), a.view(torch.int32))


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_every_bottleneck_and_the_fpn_meet_the_running_bound_in_the_16_bit_types(trunks, dtype):
    """every block is fed the twin's storage-emulated input of that block, which the type holds exactly, so the pack is exact"""
    shape = case.INPUTS[1]
    (_, keep), net, trunk = case.trunk_emulated(shape, dtype), case.trunk_net(), trunks[dtype]
    worst = 0.0
    with torch.no_grad():
        for (s, i), x in [(k, v) for k, v in keep.items() if k != 'feats']:
            assert np.array_equal(ref.ref.round_to(x, dtype), x)
            want, bound = ref.bottleneck(net['stages'][s - 1][i], x, None, dtype)
            got = trunk.block(s, i)(dev(x.astype(np.float32))).cpu().numpy()
            err = np.abs(got - want)
            worst = max(worst, float((err / bound).max()))
            assert got.shape == want.shape and (err <= bound).all(), (s, i)
        print(f'bottlenecks {dtype}: largest share of the running bound = {worst:.3f}')
        feats = keep['feats']
        wants = ref.fpn(net, [(f, None) for f in feats], dtype)
        gots = trunk.fpn([dev(f.astype(np.float32)) for f in feats])
    for name, g, (v, e) in zip(dt.LEVELS, gots, wants):
        assert (report(f'fpn, whole, level {name} {dtype}', g.cpu().numpy(), v, e) <= e).all()


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_every_fpn_level_alone_meets_its_own_bound_in_the_16_bit_types(trunks, dtype):
    """per level, top-down: the lateral fed the twin's storage-emulated stage output with the twin's stored coarser lateral as its residual
    (both exactly representable), stored as rows; then the output block fed the twin's stored lateral of that level.  Every layer is held to
    the twin's bound of that ONE layer (no error carried in), which a misplaced residual cell would break"""
    (_, keep), net, trunk = case.trunk_emulated(case.INPUTS[1], dtype), case.trunk_net(), trunks[dtype]
    feats = keep['feats']
    L, B = len(feats), feats[0].shape[0]
    coarser = None
    with torch.no_grad():
        for l in range(L - 1, -1, -1):
            x = feats[l]
            assert np.array_equal(ref.ref.round_to(x, dtype), x)
            want, bound = ref.step(net['inner'][l], x, None, dtype, residual=None if coarser is None else (coarser, np.zeros_like(coarser)), stored=True)
            rows = trunk_conv_layer(dev(x.astype(np.float32)), trunk.inner[l], None if coarser is None else dev(coarser.astype(np.float32)), store='rows')
            got = rows.view(B, x.shape[2], x.shape[3], -1).permute(0, 3, 1, 2).float().cpu().numpy()
            assert (report(f'fpn lateral {l} {dtype}', got, want, bound) <= bound).all()
            out_want, out_bound = ref.step(net['outer'][l], want, None, dtype, stored=False)
            out = trunk_conv_layer(dev(want.astype(np.float32)), trunk.outer[l]).cpu().numpy()
            assert (report(f'fpn output {l} {dtype}', out, out_want, out_bound) <= out_bound).all()
            coarser = want


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
@pytest.mark.parametrize('shape', case.INPUTS, ids=str)
def test_the_16_bit_trunk_stays_within_twice_the_twins_own_storage_effect(trunks, shape, dtype):
    """the limit per level is computed here, on the CPU, from the twin alone: 2 x the largest difference the twin shows on that level between
    rounding every stored intermediate to the type and rounding none.  The device differs from the emulation only by float32 accumulation and
    by the storage roundings that flips; the limit measures a storage rounding at every element of every layer."""
    stored, _ = case.trunk_emulated(shape, dtype)
    exact, _ = case.trunk_emulated(shape, dtype, False)
    with torch.no_grad():
        got = trunks[dtype](dev(case.trunk_images(shape)))
    for name, g, (v, _), (v0, _) in zip(dt.LEVELS, got, stored, exact):
        limit = 2 * float(np.abs(v - v0).max())
        err = float(np.abs(g.cpu().numpy() - v).max())
        print(f'level {name} {dtype} {shape}: max |device - emulation| = {err:.3e}, limit = {limit:.3e}, share = {err / limit:.3f}')
        assert limit > 0 and err <= limit


def test_the_trunk_is_inference_only(trunks):
    x = dev(case.trunk_images(case.INPUTS[0]))
    with pytest.raises(RuntimeError, match='inference only'):
        trunks['float32'](x.clone().requires_grad_())
    with torch.no_grad():
        assert trunks['float32'](x.clone().requires_grad_())[0].requires_grad is False
    with pytest.raises(ValueError, match='torch.float32'):
        trunks['float32'](x.half())

"""The detector's heads on the GPU (csrc/kernels_dethead.hip behind cosypose_amd/detector_heads.py) against the CPU twin tests/dethead_ref.py,
which test_detector_heads_host.py holds against torch's own float64 layers.

Criterion of a single layer: |got - want| <= (K + 2) u S per output against the twin's float64 evaluation, u = 2^-24 for float32 and 2^-23 for
the 16-bit types (the twin fed the operands rounded to the type).  float32 also: BIT-equal to the twin's fmaf chain.  Whole heads: the twin's
running bound through the chained layers, and in float32 the chained chains' bits.  End to end: detections_from_features against the same call
with torch.nn modules, every decision's margin asserted first (tests/dethead_e2e.py).  Every test prints its largest error as a share of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import dethead_case as case
from cosypose_amd import DetectorHeads, HeadLayer, conv_layer
from cosypose_amd import _lib

pytestmark = pytest.mark.gpu
TORCH = {'float32': torch.float32, 'float16': torch.float16, 'bfloat16': torch.bfloat16}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def head_layer(layer, dtype):
    make = {'conv': HeadLayer.conv, 'linear': HeadLayer.linear, 'deconv': HeadLayer.deconv}[layer['kind']]
    return make(torch.from_numpy(layer['weight']), torch.from_numpy(layer['bias']), relu=layer['relu'], dtype=TORCH[dtype], device='cuda')


def report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest share of the bound = {share:.3f}')
    return err


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope='module')
def heads():
    sd = {k: torch.from_numpy(v) for k, v in case.head_weights().items()}
    return {d: DetectorHeads.from_state_dict(sd, dtype=TORCH[d], device='cuda') for d in case.DTYPES}


def test_the_library_takes_its_paths_where_the_cases_expect_them():
    assert _lib.lib().cosy_head_big_rows() == case.BIG_ROWS and _lib.lib().cosy_head_max_tile_rows() == case.TILE_ROWS


# ---- single layers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', case.DTYPES)
@pytest.mark.parametrize('c', case.CASES, ids=case.case_id)
def test_a_layer_meets_the_float64_bound_and_in_float32_the_chains_bits(c, dtype):
    layer, x = case.case_data(c)
    want, bound = case.want64(c, dtype)
    got = conv_layer(dev(x), head_layer(layer, dtype)).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    err = report(f'{case.case_id(c)} {dtype}', got, want, bound)
    assert (err <= bound).all()
    if dtype == 'float32':
        chain = case.want32(c)
        differ = int((bits(got) != bits(chain)).sum())
        print(f'  outputs whose bits differ from the fmaf chain: {differ} of {got.size}')
        assert differ == 0


# ---- non-finite inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', case.DTYPES)
def test_a_nan_reaches_exactly_its_receptive_field_and_relu_keeps_it(dtype):
    import dethead_ref as ref
    for c, where, n_nan in ((('conv3', 40, 24, True, 2, 5, 7), (1, 7, 2, 3), 24 * 9), (('linear', 392, 24, True, 5, 1, 1), (2, 100), 24)):
        layer, x = case.case_data(c)
        assert layer['relu']
        x = x.copy()
        x[where] = np.nan
        want, S, K = ref.layer64(layer, x, dtype)
        bound = (K + 2) * ref.U[dtype] * S
        got = conv_layer(dev(x), head_layer(layer, dtype)).cpu().numpy()
        assert int(np.isnan(want).sum()) == n_nan and int(np.isnan(got).sum()) == n_nan
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        err = report(f'{case.case_id(c)} {dtype} beside a NaN', got[ok], want[ok], bound[ok])
        assert (err <= bound[ok]).all()


# ---- whole heads -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_the_rpn_head_meets_the_running_bound(heads, dtype):
    feats, _, _ = case.head_inputs()
    with torch.no_grad():
        obj, dl = heads[dtype].rpn_head([dev(f) for f in feats])
    assert len(obj) == len(dl) == len(feats)
    for l, (v_o, e_o, v_d, e_d) in enumerate(case.head_wants(dtype)['rpn']):
        assert tuple(obj[l].shape) == v_o.shape and tuple(dl[l].shape) == v_d.shape and obj[l].is_contiguous() and dl[l].is_contiguous()
        assert obj[l].dtype == dl[l].dtype == torch.float32
        assert (report(f'rpn objectness level {l} {dtype}', obj[l].cpu().numpy(), v_o, e_o) <= e_o).all()
        assert (report(f'rpn deltas level {l} {dtype}', dl[l].cpu().numpy(), v_d, e_d) <= e_d).all()


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_the_box_head_meets_the_running_bound(heads, dtype):
    _, roi, _ = case.head_inputs()
    with torch.no_grad():
        cls, reg = heads[dtype].box_head(dev(roi))
        none = heads[dtype].box_head(dev(roi[:0]))
    v_c, e_c, v_r, e_r = case.head_wants(dtype)['box']
    assert tuple(cls.shape) == (6, case.K) and tuple(reg.shape) == (6, 4 * case.K)
    assert (report(f'box head class logits {dtype}', cls.cpu().numpy(), v_c, e_c) <= e_c).all()
    assert (report(f'box head regression {dtype}', reg.cpu().numpy(), v_r, e_r) <= e_r).all()
    assert tuple(none[0].shape) == (0, case.K) and tuple(none[1].shape) == (0, 4 * case.K) and none[0].is_cuda and none[0].dtype == torch.float32


@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_the_mask_head_meets_the_running_bound(heads, dtype):
    _, _, mroi = case.head_inputs()
    with torch.no_grad():
        got = heads[dtype].mask_head(dev(mroi))
        none = heads[dtype].mask_head(dev(mroi[:0]))
    v, e = case.head_wants(dtype)['mask']
    assert tuple(got.shape) == (3, case.K, 28, 28) and got.dtype == torch.float32
    assert (report(f'mask head {dtype}', got.cpu().numpy(), v, e) <= e).all()
    assert tuple(none.shape) == (0, case.K, 28, 28) and none.is_cuda and none.dtype == torch.float32


def test_the_float32_heads_hold_the_bits_of_the_chained_fmaf_chains(heads):
    """the running bound grows by sum |w| per layer and would hide a misplaced pixel behind it; in float32 every layer is the twin's fmaf chain
    and the stores between the layers are exact, so the whole head is held to the chained chains' BITS (built from modules, not a state_dict)"""
    feats, roi, mroi = case.head_inputs()
    want = case.head_bits()
    h = DetectorHeads.from_modules(*case.torch_heads(), device='cuda')
    with torch.no_grad():
        obj, dl = h.rpn_head([dev(f) for f in feats])
        cls, reg = h.box_head(dev(roi))
        mask = h.mask_head(dev(mroi))
    for l in range(len(feats)):
        assert np.array_equal(bits(torch.cat([obj[l], dl[l]], 1).cpu().numpy()), bits(want['rpn'][l]))
    assert np.array_equal(bits(torch.cat([cls, reg], 1).cpu().numpy()), bits(want['box']))
    assert np.array_equal(bits(mask.cpu().numpy()), bits(want['mask']))


@pytest.mark.parametrize('dtype', case.DTYPES)
def test_two_calls_give_equal_bits(heads, dtype):
    feats, roi, mroi = case.head_inputs()
    h = heads[dtype]
    with torch.no_grad():
        runs = []
        for _ in range(2):
            obj, dl = h.rpn_head([dev(f) for f in feats])
            runs.append([*obj, *dl, *h.box_head(dev(roi)), h.mask_head(dev(mroi))])
    for a, b in zip(*runs):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_heads_are_inference_only(heads):
    feats, roi, mroi = case.head_inputs()
    h = heads['float32']
    with pytest.raises(RuntimeError, match='inference only'):
        h.box_head(dev(roi).requires_grad_())
    with pytest.raises(RuntimeError, match='inference only'):
        h.rpn_head([dev(f).requires_grad_() for f in feats])
    with pytest.raises(RuntimeError, match='inference only'):
        h.mask_head(dev(mroi).requires_grad_())
    with torch.no_grad():
        assert h.box_head(dev(roi).requires_grad_())[0].requires_grad is False


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------------------
def test_c_abi_head_conv_refusals():
    l_ = _lib.lib()
    layer, x = case.case_data(('conv3', 8, 24, True, 2, 5, 7))
    hl = head_layer(layer, 'float32')
    rows = torch.empty((70, 8), dtype=torch.float32, device='cuda')
    assert l_.cosy_head_pack(_lib.ptr(dev(x)), _lib.ptr(rows), 2, 8, 35, _lib.COSY_F32, _lib.stream()) == 0
    assert torch.equal(rows.view(2, 35, 8), dev(x).view(2, 8, 35).transpose(1, 2))
    out = torch.full((2, 24, 5, 7), -777.0, device='cuda')

    def desc(**change):
        d = _lib.HeadLayer()
        d.x, d.w, d.bias, d.out, d.out1 = _lib.ptr(rows), _lib.ptr(hl.w), _lib.ptr(hl.bias), _lib.ptr(out), None
        d.dtype, d.ksize, d.c_in, d.c_out, d.relu, d.store, d.n_split, d.n_levels = _lib.COSY_F32, 3, 8, 24, 1, _lib.HEAD_STORE_NCHW, 24, 1
        d.row_start[0], d.row_start[1], d.H[0], d.W[0] = 0, 70, 5, 7
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d
    bad = [dict(dtype=3), dict(ksize=2), dict(c_in=12), dict(c_in=0), dict(c_out=0), dict(store=4), dict(store=-1), dict(relu=2), dict(n_split=25),
           dict(n_split=-1), dict(n_split=3), dict(n_levels=0), dict(n_levels=9), dict(row_start=(0, 1)), dict(row_start=(1, 69)), dict(H=(0, 0)),
           dict(W=(0, 6)), dict(x=None), dict(w=None), dict(bias=None), dict(out=None), dict(x=rows.data_ptr() + 4),
           dict(store=_lib.HEAD_STORE_ROWS, c_out=12), dict(store=_lib.HEAD_STORE_DECONV_ROWS), dict(store=_lib.HEAD_STORE_DECONV_NCHW, ksize=1, c_out=22),
           dict(store=_lib.HEAD_STORE_DECONV_ROWS, ksize=1, c_out=24)]
    for change in bad:
        assert l_.cosy_head_conv(ctypes.byref(desc(**change)), _lib.stream()) == -1, change
        assert l_.cosy_last_error().decode().startswith('cosy_head_conv:'), change
    assert l_.cosy_head_conv(None, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (out == -777.0).all()                                    # no refused call launched anything
    empty = desc(row_start=(1, 0), x=None, w=None, bias=None, out=None)
    assert l_.cosy_head_conv(ctypes.byref(empty), _lib.stream()) == 0          # M = 0: success, nothing launched, null pointers allowed
    for args in ((None, _lib.ptr(rows), 2, 8, 35, 0), (_lib.ptr(dev(x)), None, 2, 8, 35, 0), (_lib.ptr(dev(x)), _lib.ptr(rows), 2, 12, 35, 0),
                 (_lib.ptr(dev(x)), _lib.ptr(rows), 2, 8, 0, 0), (_lib.ptr(dev(x)), _lib.ptr(rows), -1, 8, 35, 0), (_lib.ptr(dev(x)), _lib.ptr(rows), 2, 8, 35, 5)):
        assert l_.cosy_head_pack(*args, _lib.stream()) == -1, args
    assert l_.cosy_head_pack(None, None, 0, 8, 35, 0, _lib.stream()) == 0
    assert l_.cosy_head_conv(ctypes.byref(desc()), _lib.stream()) == 0
    want, bound = case.want64(('conv3', 8, 24, True, 2, 5, 7), 'float32')
    assert (np.abs(out.cpu().numpy() - want) <= bound).all()


# ---- features -> detections ------------------------------------------------------------------------------------------------------------
GRID = [(5, 7), (3, 4), (1, 2)]
SIZES = ((32,), (64,), (128,))
PAD, NETS, FRAME = (40, 56), [(37, 53), (40, 50)], (24, 40)
NAMES = {1: 'obj_000001', 2: 'obj_000002'}


def post_ulps(got, want):
    """|got - want| in float32 ulps of the larger coordinate of the box along the axis (section 21's measure)"""
    got, want = np.asarray(got, np.float32).reshape(-1, 2, 2), np.asarray(want, np.float32).reshape(-1, 2, 2)
    mag = np.abs(want).max(1, keepdims=True)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(mag, np.float32(1e-30)))


@pytest.mark.parametrize('output_masks', [False, True])
def test_detections_from_features_takes_the_heads_and_equals_the_twin_chain(output_masks):
    """detections_from_features with DetectorHeads (float32) against the twin chain tests/detpre_ref.py fed the twin's own heads, the float32 fmaf
    chains whose bits the device holds: the decisions on both sides see equal head outputs, so sections 21 and 22's tolerances apply to the chain
    unchanged.  A larger case (42 detections, real RPN deltas) than the comparison against torch.nn modules below can afford."""
    import detpost_ref as post
    import detpre_ref as pre
    from cosypose_amd import detections_from_features
    from cosypose_amd.io_formats import make_detections
    sd = case.chain_weights()
    rng = np.random.RandomState(21)
    feats = [rng.normal(0, 1, (2, case.CHAIN_C, H, W)).astype(np.float32) for H, W in GRID]
    rpn_np, box_np, mask_np = case.chain_twin_heads(sd)
    twin, props, per_image = pre.chain(feats, rpn_np, box_np, mask_np, NETS, PAD, [FRAME] * 2, NAMES, output_masks=output_masks,
                                       rpn_options=dict(sizes=SIZES, pre_nms_top_n=64, post_nms_top_n=20), head_options=dict(detections_per_img=100))
    heads = DetectorHeads.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, device='cuda')
    with torch.no_grad():
        got = detections_from_features([dev(f) for f in feats], heads.rpn_head, heads.box_head, heads.mask_head, NETS, PAD, [FRAME] * 2, NAMES,
                                       output_masks=output_masks, sizes=SIZES, pre_nms_top_n=64, post_nms_top_n=20, detections_per_img=100)
    assert len(twin['score']) > 3 and len(set(twin['batch_im_id'].tolist())) == 2 and len(set(twin['label'].tolist())) == 2
    scales = pre.infer_scales([f.shape[2:] for f in feats], NETS)
    s64 = np.concatenate([post.scores64(box_np(pre.multiscale_roi_align(feats, p['boxes'], np.full(len(p['boxes']), b), scales, 7, 2)[0])[0])[:, 1:]
                          .numpy().reshape(-1) for b, p in enumerate(props)])
    assert int((np.abs(s64 - 0.05) < 1e-4).sum()) == 0                         # no score too close to the threshold to call
    fed = [dict(boxes=o['boxes'], labels=[NAMES[int(l)] for l in o['labels']], scores=o['scores']) for o in per_image]
    want = make_detections(fed, device='cuda')
    assert got.infos['batch_im_id'].tolist() == want.infos['batch_im_id'].tolist() == twin['batch_im_id'].tolist()
    assert got.infos['label'].tolist() == want.infos['label'].tolist()
    assert np.abs(got.infos['score'].values / want.infos['score'].values - 1).max() <= (3 + 4 + 16) * 2.0 ** -24 * 2
    assert post_ulps(got.bboxes.cpu().numpy(), want.bboxes.cpu().numpy()).max() <= 5           # section 21: 4 of the decode, 1 of the step to the frame
    assert hasattr(got, 'masks') == output_masks
    if output_masks:
        boxes_net = np.array([per_image[b]['boxes_net'][j] for b, j in twin['rows']], np.float32).reshape(-1, 4)
        labels = np.array([per_image[b]['labels'][j] for b, j in twin['rows']], np.int64)
        roi = pre.multiscale_roi_align(feats, boxes_net, twin['batch_im_id'], scales, 14, 2)[0]
        v64, inside = post.paste_values(mask_np(roi), twin['bboxes'], labels, FRAME, torch.float64)
        close = ((v64 - 0.8).abs() <= 1e-5).numpy() & inside.numpy()
        D = len(labels)
        assert (close.reshape(D, -1).sum(1) <= 1e-3 * inside.numpy().reshape(D, -1).sum(1)).all()      # the exclusion cap, on the twin alone
        masks = got.masks.cpu().numpy()
        assert masks.dtype == bool and masks.shape == (D,) + FRAME and twin['masks'].any()
        assert not ((masks != twin['masks']) & ~close).any()


def test_detections_from_features_equal_with_the_torch_modules_under_asserted_margins():
    """detections_from_features with DetectorHeads against the same call with the equivalent torch.nn modules on the device, on the seeded
    2-frame case of tests/dethead_e2e.py.  That module computes on the CPU, from the twins and the heads' running bounds, how far every
    decision of the chain lies from its threshold in units of what the heads' bound can move it (top-k boundary, NMS IoU and order, score
    threshold, small-box limit, mask box truncation, mask threshold); the seed was chosen there so that every margin exceeds 100, and the
    margin is asserted here before anything runs.  Then: equal kept sets and labels, boxes within section 21's 4 ulps, equal masks."""
    import dethead_e2e as e2e
    from cosypose_amd import detections_from_features
    margins, info = e2e.margins(e2e.SEED)
    for k, v in sorted(margins.items()):
        print(f'margin of {k}: {v:.1f} x the bound')
    print(info)
    assert info['detections'] > 3 and info['images'] == 2 and info['labels'] == 2 and info['mask_pixels_on'] > 0
    assert min(margins.values()) > 100, margins
    sd = e2e.weights(e2e.SEED)
    feats = [dev(f) for f in e2e.features(e2e.SEED)]
    heads = DetectorHeads.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, device='cuda')
    rpn, box_head, box_pred, mask_head, mask_pred = case.torch_heads(sd, device='cuda')
    options = dict(output_masks=True, sizes=e2e.SIZES, pre_nms_top_n=e2e.PRE, post_nms_top_n=e2e.POST, detections_per_img=e2e.PER_IMG,
                   score_thresh=e2e.SCORE_TH, nms_thresh=e2e.NMS_TH, rpn_nms_thresh=e2e.RPN_NMS_TH, mask_th=e2e.MASK_TH)
    with torch.no_grad():
        got = detections_from_features(feats, heads.rpn_head, heads.box_head, heads.mask_head, e2e.NETS, e2e.PAD, [e2e.FRAME] * 2, e2e.NAMES, **options)
        want = detections_from_features(feats, rpn, lambda r: box_pred(box_head(r)), lambda r: mask_pred(mask_head(r)), e2e.NETS, e2e.PAD,
                                        [e2e.FRAME] * 2, e2e.NAMES, **options)

    def canonical(d):
        """the detections in an order that does not depend on the scores' last bits: image, label, box to 0.01 px"""
        boxes = d.bboxes.cpu().numpy()
        keys = [(int(i), str(l)) + tuple(np.round(b, 2).tolist()) for i, l, b in zip(d.infos['batch_im_id'], d.infos['label'], boxes)]
        order = sorted(range(len(keys)), key=keys.__getitem__)
        return [keys[i][:2] for i in order], boxes[order], d.infos['score'].values[order], d.masks.cpu().numpy()[order]
    g, w = canonical(got), canonical(want)
    assert len(g[0]) == info['detections'] and g[0] == w[0]                     # equal kept sets and labels, and the twin's count
    ulps = post_ulps(g[1], w[1])
    print(f'boxes: largest difference {float(ulps.max()):.2f} ulps; scores: {float(np.abs(g[2] - w[2]).max()):.2e}; mask pixels on: {int(g[3].sum())}')
    assert ulps.max() <= 4
    assert g[3].dtype == bool and g[3].any() and np.array_equal(g[3], w[3])

"""CPU tests of the detector's input side (cosypose_amd/detector_input.py, csrc/kernels_detin.hip): the size rule by
hand, the pixel table against the installed torch bit for bit, the numpy twin tests/detin_ref.py against the installed torch -- nearest and
boxes equal, the bilinear image within the derived per-pixel bound of detin_ref.bilinear_bound, with 1 and with 2 threads -- the host
tables of the package against the twin's, the refusals that need no device and no library, and the C ABI."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detin_ref as ref
from conftest import REPO

F32 = np.float32
# (h, w, min_size, max_size) -> (nh, nw): the single-frame cases of tests/test_detector_input.py
CASES = {(48, 64, 48, 64): (48, 64), (54, 72, 48, 64): (48, 64), (45, 60, 48, 64): (48, 64), (96, 128, 48, 64): (48, 64),
         (30, 100, 48, 64): (19, 64), (49, 70, 32, 64): (31, 45), (5, 7, 5, 7): (5, 7), (1, 1, 1, 1): (1, 1)}
BILINEAR_ONLY = {(480, 640, 540, 720): (540, 720), (47, 60, 48, 64): (47, 61)}      # weights that differ most from torch's; the other quirk


def frame_of(h, w, seed=0):
    return np.random.RandomState(seed + 131 * h + w).randint(0, 256, (3, h, w)).astype(np.uint8)


def test_size_rule_by_hand():
    from cosypose_amd import detector_input as di
    for fn in (ref.network_size, di.network_size):
        assert fn(480, 640, 480, 640) == (480, 640)                             # the reference's configuration: unchanged
        assert fn(96, 128, 48, 64) == (48, 64) and fn(45, 60, 48, 64) == (48, 64)    # the min branch, down and up
        assert fn(30, 100, 48, 64) == (19, 64)                                  # the max branch: 100 * 1.6 > 64, s = 0.64, floor(19.2)
        # the floor's quirk: s = 32 / 49, 70 * s = 45.7 <= 64 so the min branch stays, and 49 * (32 / 49) = 31.999999999999996 in doubles
        assert 49.0 * (32.0 / 49.0) < 32.0 and fn(49, 70, 32, 64) == (31, 45)
        assert 47.0 * (48.0 / 47.0) < 48.0 and fn(47, 60, 48, 64)[0] == 47
        assert fn(480, 640, 800, 1333) == (800, 1066)                           # floor(1066.67): torch 1.3's floor, not a later round
        for case, want in {**CASES, **BILINEAR_ONLY}.items():
            assert fn(*case) == want, case
    for fn in (ref.padded_size, di.padded_size):
        assert fn([(31, 45)], 32) == (32, 64) and fn([(48, 64), (19, 64), (31, 45)], 32) == (64, 64)
        assert fn([(31, 45), (19, 64)], 1) == (31, 64) and fn([(48, 64), (5, 7)], 64) == (64, 64) and fn([(800, 1066)], 32) == (800, 1088)


@pytest.mark.parametrize('mean,std', [(ref.MEAN, ref.STD), ((0.0, 0.0, 0.0), (1.0, 0.5, 2.0)), ((0.3, 0.6, 0.9), (0.1, 0.25, 0.7))])
def test_pixel_table_holds_torchs_bits(mean, std):
    from cosypose_amd import detector_input as di
    u = torch.arange(256, dtype=torch.uint8)[None, :, None].expand(3, 256, 1)
    m, s = torch.tensor(mean, dtype=torch.float32)[:, None, None], torch.tensor(std, dtype=torch.float32)[:, None, None]
    want = ((u.float() / 255 - m) / s).numpy().reshape(3, 256)
    for table in (ref.pixel_table(mean, std), di.pixel_table(mean, std)):
        assert table.dtype == F32 and np.array_equal(table.view(np.int32), want.view(np.int32))
    assert not di.pixel_table(mean, std).flags.writeable
    if mean == ref.MEAN:
        assert 2.63 < np.abs(want).max() < 2.65
    with pytest.raises(ValueError, match='not finite'):
        di.pixel_table((0, 0, 0), (1, 0, 1))
    with pytest.raises(ValueError, match='three numbers'):
        di.pixel_table((0, 0), (1, 1, 1))


def test_host_tables_and_ratios_equal_the_twin():
    from cosypose_amd import detector_input as di
    from cosypose_amd import frames
    for (h, w, _, _), (nh, nw) in {**CASES, **BILINEAR_ONLY}.items():
        for n_in, n_out in ((h, nh), (w, nw)):
            taps, nearest = frames.axis_tables(n_in, n_out)
            want_taps, want_nearest = ref.axis_ints(n_in, n_out)
            assert np.array_equal(taps, want_taps) and np.array_equal(nearest, want_nearest)
        rw, rh = di.box_ratios(h, w, nh, nw)
        assert rw.dtype == F32 and rh.dtype == F32 and rw == F32(nw / w) and rh == F32(nh / h)


@pytest.mark.parametrize('case', list(CASES), ids=lambda c: f'{c[0]}x{c[1]}_at_{c[2]}_{c[3]}')
def test_twin_nearest_and_boxes_equal_torch(case):
    h, w, _, _ = case
    nh, nw = CASES[case]
    rs = np.random.RandomState(5)
    m = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
    want = F.interpolate(torch.from_numpy(m)[None].float(), size=(nh, nw))[0].byte().numpy()
    assert np.array_equal(ref.masks(m, nh, nw), want)
    b = np.concatenate([rs.uniform(-20, 120, (6, 4)), [[3, 4, 3, 9], [0, 0, 0, 0], [-5.5, -1, -2, 7]]]).astype(F32)
    ratio_h, ratio_w = float(nh) / float(h), float(nw) / float(w)              # resize_boxes: Python floats times float32 tensors
    t = torch.from_numpy(b)
    want_b = torch.stack((t[:, 0] * ratio_w, t[:, 1] * ratio_h, t[:, 2] * ratio_w, t[:, 3] * ratio_h), dim=1).numpy()
    assert np.array_equal(ref.boxes(b, h, w, nh, nw).view(np.int32), want_b.view(np.int32))


@pytest.mark.parametrize('threads', [1, 2])
def test_twin_image_within_the_derived_bound_of_torch(threads):
    table = ref.pixel_table()
    M = float(np.abs(table).max())
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        worst, worst64, worst_weights = 0.0, 0.0, 0.0
        for (h, w, _, _), (nh, nw) in {**CASES, **BILINEAR_ONLY}.items():
            f = frame_of(h, w)
            x = torch.from_numpy(ref.pixels(f, table))
            want = F.interpolate(x[None], size=(nh, nw), mode='bilinear', align_corners=False)[0].numpy()
            got = ref.image(f, nh, nw, table)
            assert got.dtype == F32 and got.shape == (3, nh, nw)
            bound, rounding, weights = ref.bilinear_bound(f, nh, nw, table)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            err64 = np.abs(got.astype(np.float64) - ref.image_float64(f, nh, nw, table))
            own = 6 * ref.U * M * (1 + 2 * ref.U)                              # this side's share of the rounding term: its six operations
            share, share64 = float((err / bound).max()), float(err64.max() / own)
            print(f'{h}x{w} -> {nh}x{nw}, {threads} threads: |twin - torch| / bound = {share:.3f} (largest error {err.max() / (ref.U * M):.1f} u M, '
                  f'weight term up to {weights.max() / (ref.U * M):.1f} u M); |twin - float64| / (6 u M) = {share64:.3f}; '
                  f'{int((got != want).sum())} floats differ')
            assert (err <= bound).all() and (err64 <= own).all()
            if (h, w) == (nh, nw):
                assert np.array_equal(got.view(np.int32), want.view(np.int32))  # scale 1: the two routes agree to the bit
                assert np.array_equal(got.view(np.int32), ref.pixels(f, table).view(np.int32))     # ... and with p00, the one-tap path
            worst, worst64, worst_weights = max(worst, share), max(worst64, share64), max(worst_weights, float(weights.max() / (ref.U * M)))
        print(f'{threads} threads: largest share of the bound {worst:.3f}, of the float64 bound {worst64:.3f}')
    finally:
        torch.set_num_threads(before)


def test_twin_pads_with_positive_zero_and_passes_keys_through():
    frames = [frame_of(49, 70), frame_of(48, 64), frame_of(5, 7)]
    label = object()
    m = np.ones((2, 48, 64), np.uint8)
    targets = [dict(boxes=np.zeros((0, 4), F32), masks=np.zeros((0, 49, 70), np.uint8)), dict(boxes=np.ones((2, 4), F32), masks=m, labels=label),
               dict(boxes=np.ones((1, 4), F32))]
    out = ref.transform(frames, targets, min_size=[32, 48, 5], max_size=64)
    assert out['net_sizes'] == [(31, 45), (48, 64), (5, 7)] and out['padded_size'] == (64, 64) and out['original_sizes'] == [(49, 70), (48, 64), (5, 7)]
    bits = out['images'].view(np.uint32)
    assert not bits[0, :, 31:].any() and not bits[0, :, :, 45:].any() and not bits[2, :, 5:].any() and not bits[2, :, :, 7:].any()
    assert out['targets'][1]['masks'] is m and out['targets'][1]['labels'] is label and out['targets'][0]['masks'].shape == (0, 31, 45)
    assert 'masks' not in out['targets'][2]


def test_refusals_before_the_library_loads(monkeypatch):
    from cosypose_amd import _lib, detector_input

    def no_library():
        raise AssertionError('the library must not be loaded for a refusal')
    monkeypatch.setattr(_lib, 'lib', no_library)
    good = torch.zeros((3, 6, 8), dtype=torch.uint8)
    boxes = torch.zeros((2, 4))
    with pytest.raises(ValueError, match='frame 1 is torch.float32'):
        detector_input([good, good.float()])
    with pytest.raises(ValueError, match='frame 0 must have 3 channels'):
        detector_input([torch.zeros((2, 6, 8), dtype=torch.uint8)])
    with pytest.raises(ValueError, match='frame 0 must be'):
        detector_input([torch.zeros((6, 8), dtype=torch.uint8)])
    with pytest.raises(ValueError, match='at least one frame'):
        detector_input([])
    with pytest.raises(ValueError, match='2 images, got 1'):
        detector_input([good, good], [dict(boxes=boxes)])
    with pytest.raises(NotImplementedError, match='keypoints'):
        detector_input([good], [dict(boxes=boxes, keypoints=torch.zeros((2, 17, 3)))])
    with pytest.raises(ValueError, match=r'frame 0 of 6x800 would reach the network as 0x64'):
        detector_input([torch.zeros((3, 6, 800), dtype=torch.uint8)], min_size=48, max_size=64)
    with pytest.raises(ValueError, match=r'masks are \(5, 8\), its frame is \(6, 8\)'):
        detector_input([good], [dict(boxes=boxes, masks=torch.zeros((2, 5, 8), dtype=torch.uint8))])
    with pytest.raises(ValueError, match='one mask per box'):
        detector_input([good], [dict(boxes=boxes, masks=torch.zeros((3, 6, 8), dtype=torch.uint8))])
    with pytest.raises(ValueError, match='boxes must be'):
        detector_input([good], [dict(boxes=boxes.double())])
    with pytest.raises(ValueError, match='min_size'):
        detector_input([good, good], min_size=[48])
    with pytest.raises(ValueError, match='size_divisible'):
        detector_input([good], size_divisible=0)
    with pytest.raises(_lib.CosyHipError, match='ROCm device only'):            # everything is in order but the side the frame lives on
        detector_input([good])


def test_c_abi_exports_the_entry_point():
    import cosypose_amd
    from cosypose_amd import _lib, build
    from cosypose_amd import detector_input as di
    # test_c_abi.py: EXPORTS, the header and the built library name the same entry points; cosy_detin_item_t field by field, COSY_DETIN_ONE_TAP
    # and the twelve arguments of the signature
    assert 'cosy_detector_input' in _lib.EXPORTS
    assert 'kernels_detin.hip' in build.SOURCES and '-ffp-contract=off' in build.FILE_FLAGS['kernels_detin.hip']
    assert (REPO / 'cosypose_amd' / 'csrc' / 'kernels_detin.hip').exists()
    assert callable(cosypose_amd.detector_input) and cosypose_amd.detector_input.detector_input is di.detector_input
    assert cosypose_amd.detections_from_frames is di.detections_from_frames
    assert cosypose_amd.detector_losses_from_frames is di.detector_losses_from_frames

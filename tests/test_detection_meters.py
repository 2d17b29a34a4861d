"""The detection side on the GPU (csrc/kernels_det.hip behind cosypose_amd/mask_ops.py and cosypose_amd/detection_meters.py).

Every comparison is exact.  Yardsticks: tests/det_ref.py, the numpy twins that test_detection_meters_host.py holds against what the
reference recorded (one np.where per id; IoU in np.float32, one operation at a time), and tests/golden/reference_golden_det.npz
itself (the reference's own boxes on the edge masks, its IoUs, tables and summaries).  The IoU kernels round every operation to
float32 on its own, as numpy and torch do, so their results are compared as bits would be: np.array_equal with equal_nan.  The
meter's float64 summary values are compared to 1e-12 (float64 on both sides, the same operations)."""
import numpy as np
import pandas as pd
import pytest
import torch

import det_meter_case as dc
import det_ref
from cosypose_amd import DetectionMeter, box_iou, make_detections_from_segmentation, mask_instance_stats
from cosypose_amd.detection_meters import box_iou_pairs
from cosypose_amd.mask_ops import detection_targets, instance_masks, visible_ids
from cosypose_amd.tensor_collection import PandasTensorCollection

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- box IoU -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 4097])
def test_box_iou_pairs_equals_the_twin(N):
    a, b = det_ref.boxes(N + 1, N)
    got = box_iou_pairs(dev(a), dev(b)).cpu().numpy()
    want = det_ref.box_iou_pairs(a, b)
    assert got.shape == (N,) and got.dtype == np.float32
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:10]
    if N >= 63:          # every special case is in, and the NaN ones are NaN
        assert np.isnan(got[5]) and np.isnan(got[10]) and np.isnan(got[11]) and got[0] == 1 and got[2] == 0


@pytest.mark.parametrize('N,M', [(0, 5), (5, 0), (1, 1), (65, 129)])
def test_box_iou_matrix_equals_the_twin(N, M):
    a, _ = det_ref.boxes(7, N)
    _, b = det_ref.boxes(7, M)
    if N and M:
        b[0] = a[0]
    got = box_iou(dev(a), dev(b)).cpu().numpy()
    assert got.shape == (N, M) and got.dtype == np.float32
    assert np.array_equal(got, det_ref.box_iou(a, b), equal_nan=True)
    if (N, M) == (65, 129):
        assert np.isnan(got).any() and (got == 0).any() and (got > 0.5).any()
        ea, eb = det_ref.edge_boxes()                   # the pair kernel is the matrix's diagonal; an unaligned view takes the scalar loads
        pairs = box_iou_pairs(dev(ea), dev(eb)).cpu().numpy()
        assert np.array_equal(pairs, np.diagonal(box_iou(dev(ea), dev(eb)).cpu().numpy()), equal_nan=True)
        flat = torch.zeros(4 * len(ea) + 1, device='cuda')
        flat[1:] = dev(ea).reshape(-1)
        assert np.array_equal(box_iou_pairs(flat[1:].view(-1, 4), dev(eb)).cpu().numpy(), pairs, equal_nan=True)


# ---- instance statistics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', det_ref.FRAMES)
def test_mask_instance_stats_equals_the_twin_and_the_reference(H, W):
    masks = det_ref.edge_masks(H, W)
    want = det_ref.instance_stats(masks, 256)
    got = mask_instance_stats(dev(masks))
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 256, 5)
    assert np.array_equal(got.cpu().numpy(), want), (H, W)
    if H * W >= 256:
        assert (want[0, :, 0] > 0).all()                                                     # all 256 ids present
    assert np.flatnonzero(want[1, :, 0]).tolist() == [7]                                      # a single id
    assert want[2, 9].tolist()[1:] == [0, 0, W - 1, H - 1] and want[2, 9, 0] <= 4             # an id at the four corner pixels only
    # the reference's own boxes (the fixture), through the reference's function
    dets = make_detections_from_segmentation(dev(masks))
    rows = np.array([(b, i, *box.tolist()) for b, d in enumerate(dets) for i, box in d.items()], dtype=np.int64).reshape(-1, 6)
    assert np.array_equal(rows, dc.golden()[f'seg/{H}x{W}'])
    assert all(list(d) == sorted(d) for d in dets) and all(v.dtype == torch.int64 and v.is_cuda for d in dets for v in d.values())
    assert [v.tolist() for v in visible_ids(dev(masks))] == [sorted(i for i in d if i > 0) for d in dets]
    # bool masks are read as uint8; an image alone gives what it gives in the batch; two calls give the same bytes
    assert np.array_equal(mask_instance_stats(dev(masks > 0)).cpu().numpy(), det_ref.instance_stats((masks > 0).astype(np.uint8), 256))
    for b in range(3):
        assert np.array_equal(mask_instance_stats(dev(masks[b])).cpu().numpy()[0], want[b]), (H, W, b)
    assert torch.equal(mask_instance_stats(dev(masks)), got)


def test_mask_instance_stats_across_workgroups():
    """a workgroup covers 16384 pixels of a plane: 131 x 257 takes three per image, whose tables meet in the global atomics"""
    rs = np.random.RandomState(11)
    masks = rs.randint(0, 256, (2, 131, 257)).astype(np.uint8)
    masks[0, 40:100, 30:200] = 3                    # long runs, which cross slots and threads
    masks[1] = np.where(rs.uniform(size=(131, 257)) < 0.5, 17, masks[1])
    masks[1, 130, 256] = 201                        # the last pixel of the last workgroup
    masks[1][masks[1] == 77] = 0
    want = det_ref.instance_stats(masks, 256)
    assert want[1, 77].tolist() == [0, -1, -1, -1, -1]
    assert np.array_equal(mask_instance_stats(dev(masks)).cpu().numpy(), want)
    m32 = masks.astype(np.int32) * 4 - 1
    assert np.array_equal(mask_instance_stats(dev(m32), 1024).cpu().numpy(), det_ref.instance_stats(m32, 1024))


@pytest.mark.parametrize('n_ids', [1, 7, 256, 1024])
def test_mask_instance_stats_int32_skips_values_outside_the_table(n_ids):
    for H, W in det_ref.FRAMES:
        masks = det_ref.edge_masks_i32(H, W)
        assert H * W < 8 or (masks.min() == -1 and masks.max() >= n_ids)
        got = mask_instance_stats(dev(masks), n_ids).cpu().numpy()
        assert np.array_equal(got, det_ref.instance_stats(masks, n_ids)), (H, W, n_ids)
    ids = np.array([[[0, 255, 256, 1023, 1024, -1, 2 ** 31 - 1, -2 ** 31]]], dtype=np.int32)      # ids 0 and 255, and both ends of int32
    assert np.array_equal(mask_instance_stats(dev(ids), n_ids).cpu().numpy(), det_ref.instance_stats(ids, n_ids))


def test_mask_instance_stats_from_an_odd_byte_offset():
    """the planes start at odd addresses and W is odd: the wide loads take the aligned middle only"""
    for H, W in ((37, 53), (67, 131), (3, 5)):
        masks = det_ref.edge_masks(H, W)
        for offset in (1, 3, 15):
            buffer = torch.full((masks.size + 64,), 200, dtype=torch.uint8, device='cuda')     # id 200 all around: a read outside the view shows
            view = buffer[offset:offset + masks.size].view(3, H, W)
            view.copy_(dev(masks))
            assert view.data_ptr() % 16 == offset and view.is_contiguous()
            assert np.array_equal(mask_instance_stats(view).cpu().numpy(), det_ref.instance_stats(masks, 256)), (H, W, offset)
            rows = [(0, 9), (2, 9), (1, 7), (2, 255)]
            got = instance_masks(view, [r[0] for r in rows], [r[1] for r in rows]).cpu().numpy()
            assert np.array_equal(got, np.stack([masks[b] == i for b, i in rows]).astype(np.uint8))


# ---- binary masks and detection targets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', det_ref.FRAMES + ((32, 48),))          # 32 x 48: planes of a multiple of 16 pixels, the wide kernel
def test_instance_masks_equal_numpy(H, W):
    masks = det_ref.edge_masks(H, W)
    rows = [(b, i) for b in range(3) for i in (0, 7, 9, 255, int(masks[b].flat[0]))] + [(3, 7), (-1, 7), (1, 256), (1, -1)]
    got = instance_masks(dev(masks), [r[0] for r in rows], [r[1] for r in rows])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(rows), H, W)
    want = np.stack([masks[b] == i if 0 <= b < 3 else np.zeros((H, W), bool) for b, i in rows]).astype(np.uint8)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not want[-4:].any() and want[:15].any()                      # an image index out of range gives zeros
    m32 = det_ref.edge_masks_i32(H, W)
    rows32 = [(0, -1), (1, 34), (2, 1274), (2, 44), (5, 34)]
    got = instance_masks(dev(m32), torch.tensor([r[0] for r in rows32]), torch.tensor([r[1] for r in rows32]).cuda()).cpu().numpy()
    assert np.array_equal(got, np.stack([m32[b] == i if b < 3 else np.zeros((H, W), bool) for b, i in rows32]).astype(np.uint8))
    assert tuple(instance_masks(dev(masks), [], []).shape) == (0, H, W)                           # N = 0


def test_detection_targets_keep_rule_and_contents():
    masks = np.zeros((2, 40, 60), dtype=np.uint8)
    masks[0, 5:11, 10:21] = 1          # inclusive box 10, 5, 20, 10: area (20 - 10) * (10 - 5) = 50
    masks[0, 20:26, 10:22] = 2         # area 11 * 5 = 55
    masks[1, 0:40, 0:60] = 3           # area 59 * 39
    masks[1, 7, 7] = 4                 # one pixel: area 0
    image_ids, ids = [0, 0, 1, 1, 1], [1, 2, 3, 4, 9]
    for min_area, keep in ((50, [False, True, True, False, False]), (49, [True, True, True, False, False]), (55, [False, False, True, False, False])):
        t = detection_targets(dev(masks), image_ids, ids, min_area=min_area)
        assert t['keep'].cpu().tolist() == keep, min_area                # strictly greater, as the reference has it
        kept = [n for n, k in enumerate(keep) if k]
        boxes = {0: [10, 5, 20, 10], 1: [10, 20, 21, 25], 2: [0, 0, 59, 39]}
        assert t['boxes'].dtype == torch.float32 and t['boxes'].cpu().tolist() == [boxes[n] for n in kept]
        assert t['area'].cpu().tolist() == [(boxes[n][2] - boxes[n][0]) * (boxes[n][3] - boxes[n][1]) for n in kept]
        want = np.stack([masks[image_ids[n]] == ids[n] for n in kept]).astype(np.uint8)
        assert t['masks'].dtype == torch.uint8 and np.array_equal(t['masks'].cpu().numpy(), want)
    t = detection_targets(dev(masks), [], [])
    assert tuple(t['masks'].shape) == (0, 40, 60) and tuple(t['boxes'].shape) == (0, 4) and t['keep'].numel() == 0


# ---- the meter ---------------------------------------------------------------------------------------------------------------------------
def _collections(scene_id, device='cuda'):
    gt_infos, gt_boxes, pred_infos, pred_boxes = dc.frames(scene_id)
    return (PandasTensorCollection(pred_infos, bboxes=torch.from_numpy(pred_boxes).to(device)),
            PandasTensorCollection(gt_infos, bboxes=torch.from_numpy(gt_boxes).to(device)))


@pytest.mark.parametrize('name', dc.configs())
def test_detection_meter_equals_the_reference(name):
    g, cfg = dc.golden(), dc.config(name)
    meter = DetectionMeter(**cfg)
    for a, scene_id in enumerate(g['scene_ids']):
        pred, gt = _collections(scene_id, device='cuda' if a == 0 else 'cpu')          # host boxes are moved to the device
        meter.add(pred, gt)
        assert np.array_equal(meter.last_candidates['ious'].view(np.uint32), g[f'{name}/{a}/iou'].view(np.uint32)), (name, a)
        dc.check_tables(name, a, meter.datas['matches_df'][a], meter.datas['gt_df'][a], meter.datas['pred_df'][a])
    summary, dfs = meter.summary()
    dc.check_summary(name, summary, dfs)
    meter.reset()
    assert not meter.datas


def test_detection_meter_with_nothing_to_match():
    pred, gt = _collections(3)
    none = PandasTensorCollection(pred.infos.iloc[:0].reset_index(drop=True), bboxes=pred.bboxes[:0])
    meter = DetectionMeter()
    meter.add(none, gt)                                                  # an empty prediction set
    summary, _ = meter.summary()
    assert summary['n_pred'] == 0 and summary['n_matched'] == 0 and summary['n_gt'] == len(gt.infos) and summary['AP'] == 0. and summary['mAP'] == 0.
    assert summary['pred_matched_ratio'] == 0 and summary['iou_valid_recall'] == 0
    other = pred.infos.copy()
    other['label'] = 'something_else'                                    # predictions, but no candidate pair
    meter = DetectionMeter()
    meter.add(PandasTensorCollection(other, bboxes=pred.bboxes), gt)
    summary, dfs = meter.summary()
    assert len(meter.last_candidates['ious']) == 0 and summary['n_matched'] == 0 and summary['n_pred'] > 0 and summary['AP'] == 0.
    assert not dfs['preds']['iou_valid'].any() and dfs['gt']['iou'].isna().all()

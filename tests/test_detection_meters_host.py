"""CPU tests of the detection side (cosypose_amd/detection_meters.py, cosypose_amd/mask_ops.py, csrc/kernels_det.hip): the numpy twins of
tests/det_ref.py against what the reference recorded (tests/golden/reference_golden_det.npz, written by
tests/golden/generate_golden_det.py), and the host half of the meter -- detection_tables and summarize, which need no device -- on
the recorded IoUs against every recorded table and summary value of all six configurations.  Integer and boolean columns are
compared exactly, float64 summary values to 1e-12 (float64 on both sides, the same operations)."""
import numpy as np
import pandas as pd
import pytest

import det_meter_case as dc
import det_ref
from cosypose_amd import synthetic as syn
from cosypose_amd.detection_meters import detection_tables, summarize
from cosypose_amd.pose_meters import prepare_candidates


def test_twin_boxes_equal_the_reference_on_the_edge_masks():
    g = dc.golden()
    for H, W in det_ref.FRAMES:
        want = g[f'seg/{H}x{W}']
        dets = det_ref.detections(det_ref.edge_masks(H, W), 256)
        got = np.array([(b, i, *box) for b, d in enumerate(dets) for i, box in d.items()], dtype=np.int64).reshape(-1, 6)
        assert np.array_equal(got, want), (H, W)
        assert len(dets) == 3 and len(want) > 0
    all_ids = g['seg/67x131']
    assert set(all_ids[all_ids[:, 0] == 0, 1]) == set(range(256))             # the case "all 256 ids present" is what it says
    corners = g['seg/37x53']
    assert [tuple(r[2:]) for r in corners if r[0] == 2 and r[1] == 9] == [(0, 0, 52, 36)]


def _host_adds(name):
    """prepare_candidates and detection_tables of both scenes of the fixture on the RECORDED IoUs"""
    g, cfg = dc.golden(), dc.config(name)
    out = []
    for a, scene_id in enumerate(g['scene_ids']):
        gt_infos, _, pred_infos, _ = dc.frames(scene_id)
        prep = prepare_candidates(pred_infos, gt_infos, targets=cfg['targets'], n_top=cfg['n_top'], visib_gt_min=cfg['visib_gt_min'],
                                  consider_all_predictions=cfg['consider_all_predictions'])
        out.append((prep, detection_tables(prep['cand_infos'], g[f'{name}/{a}/iou'], prep['pred_infos'], prep['gt_infos'], cfg['iou_threshold'])))
    return out


@pytest.mark.parametrize('name', dc.configs())
def test_tables_and_summary_equal_the_reference(name):
    g = dc.golden()
    assert len(dc.configs()) == 6
    tables = dict(gt=[], matches=[], preds=[])
    for a, (prep, (matches, gt, preds, kept)) in enumerate(_host_adds(name)):
        for k in ('keep_ids', 'filtered_ids'):
            assert np.array_equal(prep[k], g[f'{name}/{a}/{k}']), (name, a, k)
        assert np.array_equal(prep['gt_infos']['valid'].values.astype(bool), g[f'{name}/{a}/gt_valid'])
        assert np.array_equal(prep['cand_infos']['pred_id'].values, g[f'{name}/{a}/cand_pred_id'])
        assert np.array_equal(prep['cand_infos']['gt_id'].values, g[f'{name}/{a}/cand_gt_id'])
        assert np.array_equal(kept['cand_id'].values, g[f'{name}/{a}/kept_cand_id'])
        assert np.array_equal(matches['cand_id'].values, g[f'{name}/{a}/match_cand_id'])
        dc.check_tables(name, a, matches, gt, preds)
        assert 'visib_fract' not in gt                                        # the reference's line 112
        tables['gt'].append(gt); tables['matches'].append(matches); tables['preds'].append(preds)
    cat = {k: pd.concat(v, ignore_index=True) for k, v in tables.items()}
    summary, dfs = summarize(cat['gt'], cat['matches'], cat['preds'], n_top=dc.config(name)['n_top'])
    dc.check_summary(name, summary, dfs)


def test_iou_twin_equals_the_reference_bit_for_bit():
    g = dc.golden()
    n = 0
    for name in dc.configs():
        for a, scene_id in enumerate(g['scene_ids']):
            _, gt_boxes, _, pred_boxes = dc.frames(scene_id)
            pred = pred_boxes[g[f'{name}/{a}/keep_ids']][g[f'{name}/{a}/filtered_ids']][g[f'{name}/{a}/cand_pred_id']]
            gt = gt_boxes[g[f'{name}/{a}/cand_gt_id']]
            want = g[f'{name}/{a}/iou']
            assert want.dtype == np.float32
            assert np.array_equal(det_ref.box_iou_pairs(pred, gt).view(np.uint32), want.view(np.uint32)), (name, a)
            assert np.array_equal(np.diagonal(det_ref.box_iou(pred, gt)).view(np.uint32), want.view(np.uint32)), (name, a)
            n += len(want)
    assert n > 500
    a, b = det_ref.edge_boxes()                                               # and the special cases are what their comments say
    iou = det_ref.box_iou_pairs(a, b)
    assert iou[0] == 1 and iou[1] == 0 and iou[2] == 0 and iou[4] == 0 and np.isnan(iou[5]) and np.isnan(iou[10]) and np.isnan(iou[11])
    assert abs(iou[3] - 35 * 40 / 1e4) < 1e-7


def test_summary_without_a_valid_ground_truth_does_what_the_reference_does():
    assert dc.golden()['zero_valid_raises'].item() is True
    (_, (matches, gt, preds, _)), _ = _host_adds('default')
    gt = gt.copy()
    gt['valid'] = False
    with np.errstate(all='ignore'), pytest.raises(ZeroDivisionError):
        summarize(gt, matches, preds)


def test_quirks_of_the_summary():
    """pred_matched_ratio is predictions per match; a label's AP is scaled by n_tp / n_gt; labels without a true positive stay out of mAP"""
    tables = [t for _, t in _host_adds('default')]
    cat = [pd.concat([t[k] for t in tables], ignore_index=True) for k in (1, 0, 2)]
    summary, dfs = summarize(*cat)
    assert summary['pred_matched_ratio'] == summary['n_pred'] / summary['n_matched'] > 1
    aps = {l: np.unique(df['AP']).item() for l, df in dfs['ap'].items() if l != 'all'}
    assert summary['mAP'] == np.mean(list(aps.values())) and len(aps) == 5
    assert len(dfs['ap']['all']) == summary['n_pred']
    n_top1, _ = summarize(*cat, n_top=1)
    groups = cat[0].groupby(dc.GROUP_KEYS)['valid'].sum()
    assert n_top1['n_gt_valid'] == int(np.minimum(1, groups).sum()) < summary['n_gt_valid']


def test_scene_and_mask_makers_are_seeded_and_as_described():
    s1, s2 = syn.make_det_scene(5), syn.make_det_scene(5)
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    assert np.array_equal(dc.golden()['pred_bboxes'], syn.make_det_scene(dc.golden()['scene_seed'].item(), scene_ids=(3, 7))['pred_bboxes'])
    assert len(np.unique(s1['pred_score'])) == len(s1['pred_score'])
    counts = pd.DataFrame(dict(s=s1['gt_scene_id'], v=s1['gt_view_id'], l=s1['gt_label'])).groupby(['s', 'v', 'l']).size()
    assert counts.max() > 1                                                    # several instances per label
    m = syn.make_instance_masks(3, 2, 48, 64, 20)
    assert m.shape == (2, 48, 64) and m.dtype == np.uint8 and m.max() <= 20 and (m == 0).any() and len(np.unique(m)) > 8
    assert np.array_equal(m, syn.make_instance_masks(3, 2, 48, 64, 20))

"""What test_detection_meters_host.py and test_detection_meters.py share: the fixture tests/golden/reference_golden_det.npz (written by
tests/golden/generate_golden_det.py from the reference's own DetectionMeter), the frames of its scene, and the comparison of this
package's tables and summary with the recorded ones.  A recorded table is one float64 matrix (columns, rows) with `label` as an index
into `labels`; integers and booleans are exact in float64, so `np.array_equal` on the matrix is an exact comparison of every column."""
import functools
import pathlib

import numpy as np
import pandas as pd

REPO = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden' / 'reference_golden_det.npz'
GROUP_KEYS = ['scene_id', 'view_id', 'label']
SUMMARY_KEYS = ('n_gt', 'n_gt_valid', 'n_pred', 'n_matched', 'matched_gt_ratio', 'pred_matched_ratio', 'iou_valid_recall', 'AP', 'mAP')
INT_KEYS = SUMMARY_KEYS[:4]
TABLE_COLUMNS = {'matches': ('scene_id', 'view_id', 'label', 'pred_inst_id', 'gt_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'),
                 'gt': ('scene_id', 'view_id', 'label', 'gt_inst_id', 'valid', 'pred_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'),
                 'preds': ('scene_id', 'view_id', 'label', 'pred_inst_id', 'score', 'iou_valid')}
# dtype kinds the reference's xr_merge leaves: a merged-in variable takes its fill value's dtype (NaN -> float64, False -> bool)
TABLE_KINDS = {'matches': dict(pred_inst_id='i', gt_inst_id='i', cand_id='i', iou='f', iou_valid='b', score='f'),
               'gt': dict(gt_inst_id='i', valid='b', pred_inst_id='f', cand_id='f', iou='f', iou_valid='b', score='f'),
               'preds': dict(pred_inst_id='i', score='f', iou_valid='b')}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def configs():
    return [str(n) for n in golden()['config_names']]


def config(name):
    g = golden()
    cfg = {k: g[f'{name}/cfg_{k}'].item() for k in ('iou_threshold', 'visib_gt_min', 'n_top', 'consider_all_predictions')}
    targets = None
    if g[f'{name}/cfg_targets'].item():
        targets = pd.DataFrame(dict(scene_id=g['targets_scene_id'], view_id=g['targets_view_id'],
                                    label=g['labels'][g['targets_label']].astype(str), inst_count=g['targets_inst_count']))
    return dict(cfg, targets=targets)


def frames(scene_id):
    """-> gt infos, gt boxes, prediction infos, prediction boxes of one scene of the fixture (numpy / pandas)"""
    g = golden()
    names = g['labels'].astype(str)
    gsel, psel = g['gt_scene_id'] == scene_id, g['pred_scene_id'] == scene_id
    gt = pd.DataFrame(dict(scene_id=g['gt_scene_id'][gsel], view_id=g['gt_view_id'][gsel], label=names[g['gt_label'][gsel]],
                           visib_fract=g['gt_visib_fract'][gsel]))
    pred = pd.DataFrame(dict(scene_id=g['pred_scene_id'][psel], view_id=g['pred_view_id'][psel], label=names[g['pred_label'][psel]],
                             score=g['pred_score'][psel]))
    return gt, g['gt_bboxes'][gsel], pred, g['pred_bboxes'][psel]


def table_matrix(frame, table):
    """a frame of this package in the fixture's form; the columns must be exactly the reference's, with its dtype kinds"""
    assert set(frame.columns) == set(TABLE_COLUMNS[table]), (table, list(frame.columns))
    for col, kind in TABLE_KINDS[table].items():
        assert frame[col].dtype.kind == kind, (table, col, frame[col].dtype)
    index = {l: n for n, l in enumerate(golden()['labels'].astype(str))}
    return np.stack([np.array([index[l] for l in frame[col]], dtype=np.float64) if col == 'label' else frame[col].values.astype(np.float64)
                     for col in TABLE_COLUMNS[table]]).reshape(len(TABLE_COLUMNS[table]), -1)


def check_tables(name, a, matches, gt, preds):
    """every column of the three tables of add number `a` of configuration `name`, exactly (NaN where the reference has NaN)"""
    g = golden()
    for table, frame in (('matches', matches), ('gt', gt), ('preds', preds)):
        got, want = table_matrix(frame, table), g[f'{name}/{a}/{table}']
        assert got.shape == want.shape, (name, a, table, got.shape, want.shape)
        for n, col in enumerate(TABLE_COLUMNS[table]):
            assert np.array_equal(got[n], want[n], equal_nan=True), (name, a, table, col)


def check_summary(name, summary, dfs):
    g = golden()
    want = dict(zip(SUMMARY_KEYS, g[f'{name}/summary']))
    assert set(summary) == set(SUMMARY_KEYS)
    for k in SUMMARY_KEYS:
        if k in INT_KEYS:
            assert summary[k] == int(want[k]) and isinstance(summary[k], int), (name, k, summary[k], want[k])
        else:
            assert abs(float(summary[k]) - want[k]) <= 1e-12, (name, k, summary[k], want[k])
    names = g['labels'].astype(str)
    labels = [names[n] for n in g[f'{name}/summary/labels']]
    ap_want = dict(zip(labels, g[f'{name}/summary/AP/labels']))
    with_tp = {l for l, v in ap_want.items() if not np.isnan(v)}
    assert set(dfs['ap']) - {'all'} == with_tp, (name, set(dfs['ap']), with_tp)
    for l in with_tp:
        assert abs(np.unique(dfs['ap'][l]['AP']).item() - ap_want[l]) <= 1e-12, (name, l)
        assert np.unique(dfs['ap'][l]['n_gt']).item() == dict(zip(labels, g[f'{name}/summary/n_gt/labels']))[l], (name, l)
    assert names[-1] not in with_tp                                       # the label the scene maker leaves without a true positive

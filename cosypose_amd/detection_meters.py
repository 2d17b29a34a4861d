"""Detection evaluation: IoU of predicted against ground-truth boxes, BOP-style greedy matching, AP / mAP / recall at an IoU
threshold.  Same surface and the same numbers as the reference's DetectionMeter
(cosypose/evaluation/meters/detection_meters.py:14-209 with meters/utils.py), quirks included; and box_iou / box_iou_pairs with
torchvision.ops.box_iou's float32 arithmetic (HIP: cosy_box_iou_matrix / cosy_box_iou_pairs), which a ROCm user has no other source of.

What runs where
  * device: ONE box_iou_pairs call for all tentative (prediction, ground truth) pairs of an `add`, where the reference builds the
    full IoU matrix of every 512-pair chunk and keeps its diagonal;
  * host, pandas / numpy: grouping and filtering (pose_meters.prepare_candidates), the threshold, the greedy matching
    (pose_meters.match_poses) and the tables (detection_tables), and everything `summary` reports (summarize).
detection_tables and summarize take numpy IoUs and frames: the host half runs (and is tested) without a device.

Tables are pandas frames with the reference's variable names as columns, as in pose_meters.py; the left merges xarray did are
pose_meters._left_fill with this meter's fill values (`iou` NaN, `iou_valid` False, `score` NaN): a merged-in variable takes the fill
value's dtype, so `pred_inst_id`, `cand_id` and `iou` are float64 in the gt table.

The reference's quirks, kept:
  * `visib_fract` never reaches the gt table: detection_meters.py:112 looks for it in the (scene, view) frame that line 63 made, which
    never has it;
  * `pred_matched_ratio` is n_pred / max(n_matched, 1) -- predictions per match, not the matched share of the predictions;
  * a label's AP is sklearn's average precision times n_tp / n_gt; `mAP` is the mean over the labels with at least one true positive
    (a label without one is left out, not counted as 0); `AP` ('all') is taken over every prediction, those of labels without any
    ground truth included;
  * with n_top > 0, n_gt of a label is the sum over its (scene, view) groups of min(n_top, valid ground truths of the group);
  * n_gt_valid == 0 (no valid ground truth at all, or nothing added): `summary` raises ZeroDivisionError at `matched_gt_ratio`, as
    the reference's lines do (recorded by tests/golden/generate_golden_det.py as `zero_valid_raises`).
Where the reference's order depends on an unstable sort (equal scores) this module is stable: the earlier row comes first.
`errors_bsz` is accepted and ignored: all pairs go in one launch.
"""
from collections import defaultdict

import numpy as np
import pandas as pd
import torch

from . import _lib
from .pose_meters import GROUP_KEYS, _left_fill, average_precision, match_poses, prepare_candidates

FILL_VALUES = {'iou': np.nan, 'iou_valid': False, 'score': np.nan}


# ---- device half -------------------------------------------------------------------------------------------------------------------
def _boxes(t, name):
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError(f'{name} must be (N,4) xyxy boxes, got {tuple(t.shape)}')
    _lib.require_device(t)
    return t.float().contiguous()


def box_iou_pairs(a, b):
    """IoU of box a[n] with box b[n]: (N,4), (N,4) xyxy -> (N) float32, the diagonal of box_iou(a, b) bit for bit"""
    a, b = _boxes(a, 'a'), _boxes(b, 'b')
    if a.shape[0] != b.shape[0]:
        raise ValueError(f'box_iou_pairs needs as many boxes in a as in b, got {a.shape[0]} and {b.shape[0]}')
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().cosy_box_iou_pairs(_lib.ptr(a), _lib.ptr(b), a.shape[0], _lib.ptr(out), _lib.stream()))
    return out


def box_iou(a, b):
    """torchvision.ops.box_iou: (N,4), (M,4) xyxy -> (N,M) float32 with torchvision's float32 arithmetic (NaN coordinates give NaN,
    two zero-area boxes at one point give NaN, inverted boxes follow the formula)"""
    a, b = _boxes(a, 'a'), _boxes(b, 'b')
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().cosy_box_iou_matrix(_lib.ptr(a), _lib.ptr(b), a.shape[0], b.shape[0], _lib.ptr(out), _lib.stream()))
    return out


# ---- the host half of `add` (detection_meters.py:102-141) --------------------------------------------------------------------------
def detection_tables(cand_infos, ious, pred_infos, gt_infos, iou_threshold):
    """cand_infos: the tentative pairs, ious: numpy array indexed by cand_id, pred_infos / gt_infos: prepare_candidates'.
    -> (matches, gt, preds) frames, (kept cand_infos) as a fourth value."""
    on_pred, on_gt = GROUP_KEYS + ['pred_inst_id'], GROUP_KEYS + ['gt_inst_id']
    ious = np.asarray(ious)
    cand_infos = cand_infos.copy()
    cand_infos['iou'] = ious
    cand_infos = cand_infos[cand_infos['iou'] >= iou_threshold].reset_index(drop=True)
    cand_infos['error'] = -cand_infos['iou']
    matched = match_poses(cand_infos)

    gt = gt_infos.loc[:, GROUP_KEYS + ['gt_inst_id', 'valid']].reset_index(drop=True).copy()       # (never visib_fract: see the module docstring)
    preds = pred_infos.loc[:, GROUP_KEYS + ['pred_inst_id', 'score']].reset_index(drop=True).copy()
    matches = matched.loc[:, GROUP_KEYS + ['pred_inst_id', 'gt_inst_id', 'cand_id']].reset_index(drop=True).copy()
    cand = matches['cand_id'].values.astype(int)
    matches['iou'] = ious[cand]
    matches['iou_valid'] = ious[cand] >= iou_threshold
    matches['score'] = _left_fill(matches, preds, on_pred, ['score'], FILL_VALUES)['score']
    for k, v in _left_fill(gt, matches, on_gt, ['pred_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'], FILL_VALUES).items():
        gt[k] = v
    preds['iou_valid'] = _left_fill(preds, matches, on_pred, ['iou_valid'], FILL_VALUES)['iou_valid']
    return matches, gt, preds, cand_infos


# ---- summary (detection_meters.py:143-209) -----------------------------------------------------------------------------------------
def summarize(gt_df, matches_df, pred_df, n_top=-1):
    """-> (summary dict, dict of frames): see DetectionMeter.summary"""
    valid_df = gt_df[gt_df['valid'].values.astype(bool)].reset_index(drop=True)
    n_gts = dict()
    if n_top > 0:
        subdf = gt_df[GROUP_KEYS + ['valid']].groupby(GROUP_KEYS).sum().reset_index()
        subdf['gt_count'] = np.minimum(n_top, subdf['valid'])
        for label, group in subdf.groupby('label'):
            n_gts[label] = group['gt_count'].sum()
    else:
        for label, n in gt_df[['label', 'valid']].groupby('label')['valid'].sum().items():
            n_gts[label] = n

    def compute_ap(label_df, label_n_gt):
        label_df = label_df.sort_values('score', ascending=False, kind='stable').reset_index(drop=True)
        label_df['n_tp'] = np.cumsum(label_df['iou_valid'].values.astype(float))
        label_df['prec'] = label_df['n_tp'] / (np.arange(len(label_df)) + 1)
        label_df['recall'] = label_df['n_tp'] / label_n_gt
        y_true = label_df['iou_valid']
        ap = average_precision(y_true, label_df['score']) * y_true.sum() / label_n_gt
        label_df['AP'] = ap
        label_df['n_gt'] = label_n_gt
        return ap, label_df

    ap_dfs = dict()
    df = pred_df[['label', 'iou_valid', 'score']]
    for label, label_n_gt in n_gts.items():
        label_df = df[(df['label'] == label).values]
        if len(label_df) and label_df['iou_valid'].sum() > 0:
            ap_dfs[label] = compute_ap(label_df, label_n_gt)[1]
    if len(ap_dfs) > 0:
        mAP = np.mean([np.unique(ap_df['AP']).item() for ap_df in ap_dfs.values()])
        AP, ap_dfs['all'] = compute_ap(df, sum(list(n_gts.values())))
    else:
        AP, mAP = 0., 0.
    n_gt_valid = int(sum(list(n_gts.values())))

    n_matched = len(matches_df)
    summary = {
        'n_gt': len(gt_df),
        'n_gt_valid': n_gt_valid,
        'n_pred': len(pred_df),
        'n_matched': n_matched,
        'matched_gt_ratio': n_matched / n_gt_valid,
        'pred_matched_ratio': len(pred_df) / max(n_matched, 1),
        'iou_valid_recall': int(valid_df['iou_valid'].sum()) / n_gt_valid,
        'AP': AP,
        'mAP': mAP,
    }
    dfs = dict(gt=gt_df, matches=matches_df, preds=pred_df, ap=ap_dfs)
    return summary, dfs


_EMPTY = {
    'gt_df': GROUP_KEYS + ['gt_inst_id', 'valid', 'pred_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'],
    'matches_df': GROUP_KEYS + ['pred_inst_id', 'gt_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'],
    'pred_df': GROUP_KEYS + ['pred_inst_id', 'score', 'iou_valid'],
}


# ---- the meter ---------------------------------------------------------------------------------------------------------------------
class DetectionMeter:
    """The reference's DetectionMeter.  pred_data / gt_data: collections with `infos` (scene_id, view_id, label; score for the
    predictions; visib_fract where visib_gt_min or targets need it) and `bboxes` (n,4) xyxy."""

    def __init__(self, iou_threshold=0.5, errors_bsz=512, consider_all_predictions=False, targets=None, visib_gt_min=-1, n_top=-1):
        self.iou_threshold = iou_threshold
        self.consider_all_predictions = consider_all_predictions
        self.targets = targets
        self.visib_gt_min = visib_gt_min
        self.errors_bsz = errors_bsz
        self.n_top = n_top
        self.reset()

    def reset(self):
        self.datas = defaultdict(list)

    def is_data_valid(self, data):
        return hasattr(data, 'bboxes') and all(k in data.infos for k in GROUP_KEYS)

    def compute_metrics(self, bbox_pred, bbox_gt):
        """IoU of len(bbox_pred) pairs -> dict of device tensors"""
        device = bbox_pred.device if bbox_pred.is_cuda else (bbox_gt.device if bbox_gt.is_cuda else 'cuda')
        return dict(iou=box_iou_pairs(bbox_pred.float().to(device), bbox_gt.float().to(device)))

    def add(self, pred_data, gt_data):
        pred_boxes_all = pred_data.bboxes.float()
        gt_boxes = gt_data.bboxes.float()
        prep = prepare_candidates(pred_data.infos, gt_data.infos, targets=self.targets, n_top=self.n_top, visib_gt_min=self.visib_gt_min,
                                  consider_all_predictions=self.consider_all_predictions)
        cand_infos = prep['cand_infos']
        ids = lambda v, t: torch.as_tensor(np.asarray(v), dtype=torch.long, device=t.device)
        filtered_boxes = pred_boxes_all[ids(prep['keep_ids'], pred_boxes_all)][ids(prep['filtered_ids'], pred_boxes_all)]
        metrics = self.compute_metrics(filtered_boxes[ids(cand_infos['pred_id'].values, filtered_boxes)],
                                       gt_boxes[ids(cand_infos['gt_id'].values, gt_boxes)])
        ious = metrics['iou'].cpu().numpy()
        matches, gt, preds, kept = detection_tables(cand_infos, ious, prep['pred_infos'], prep['gt_infos'], self.iou_threshold)
        self.last_candidates = dict(cand_infos=cand_infos, kept=kept, ious=ious)      # of this `add`, for inspection
        self.datas['gt_df'].append(gt)
        self.datas['pred_df'].append(preds)
        self.datas['matches_df'].append(matches)

    def summary(self):
        frames = {k: pd.concat(self.datas[k], axis=0, ignore_index=True) if self.datas[k] else pd.DataFrame(columns=cols)
                  for k, cols in _EMPTY.items()}
        return summarize(frames['gt_df'], frames['matches_df'], frames['pred_df'], n_top=self.n_top)

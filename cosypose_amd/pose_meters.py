"""Pose evaluation: ADD / ADD-S / ADD(-S) errors of predictions against ground truth, BOP-style matching, AUC of the error curve
and AP / mAP at 0.1 d.  Same surface and the same numbers as the reference's PoseErrorMeter
(cosypose/evaluation/meters/pose_meters.py:17-322 with meters/utils.py), quirks included.

What runs where
  * device: ONE distances.pose_errors call (HIP: cosy_pose_errors) for all tentative (prediction, ground truth) pairs of an `add`,
    each on its own object's points and with its own mode, where the reference loops over the pairs one by one;
  * host, pandas / numpy in float64: grouping and filtering (prepare_candidates), the sphere-overlap filter, the threshold filter,
    the greedy matching and the tables (match_tables), and everything `summary` reports.
The two halves are separate functions: match_tables takes the candidate table and an errors dict of numpy arrays, so the host half
runs (and is tested) without a device.

In place of the reference's xarray datasets the tables are pandas frames with the same variable names as columns; the variables
with more than one value per row (`xyz`, `TCO_xyz`: 3, `TXO_pred`: 4x4) are object columns of numpy arrays.  The left merges
xarray did (utils/xarray.py:4-42) are restated by _left_fill with the reference's fill values and result dtypes: a merged-in
variable becomes float64 (bool for `0.1d`), its missing rows inf (`norm`, `xyz`, `TCO_*`), False (`0.1d`) or NaN (all others,
the integer ids `pred_inst_id` / `cand_id` included).  average_precision and compute_auc_posecnn restate sklearn's
average_precision_score and the reference's PoseCNN AUC; nothing here imports xarray, sklearn or scipy.

Where the reference's order depends on an unstable sort (equal scores inside a (scene, view, label) group) this module is stable:
the earlier row comes first.  The means of `report_error_stats` are taken in float64 (the reference's run in float32).
"""
from collections import OrderedDict, defaultdict

import numpy as np
import pandas as pd
import torch

GROUP_KEYS = ['scene_id', 'view_id', 'label']
FILL_VALUES = {'norm': np.inf, '0.1d': False, 'xyz': np.inf, 'TCO_xyz': np.inf, 'TCO_norm': np.inf, 'obj_diameter': np.nan,
               'TXO_pred': np.nan, 'score': np.nan}
VECTOR_SHAPES = {'xyz': (3,), 'TCO_xyz': (3,), 'TXO_pred': (4, 4)}


# ---- restated metrics ------------------------------------------------------------------------------------------------------
def compute_auc_posecnn(errors):
    """Area under the accuracy-vs-error curve up to 0.1 m, scaled to [0, 1] (the YCB-Video toolbox's measure, meters/utils.py:132-152).
    Errors above 0.1 (unmatched ground truth: inf) only count in the denominator; no error at or below 0.1 (or none at all): NaN."""
    d = np.sort(np.asarray(errors, dtype=np.float64))
    n = d.shape[0]
    accuracy = np.cumsum(np.ones(n)) / n if n else np.zeros(0)
    keep = np.isfinite(d) & ~(d > 0.1)
    d, accuracy = d[keep], accuracy[keep]
    if d.size == 0:
        return np.nan
    mrec = np.concatenate(([0.], d, [0.1]))
    mpre = np.maximum.accumulate(np.concatenate(([0.], accuracy, [accuracy[-1]])))
    ids = np.where(mrec[1:] != mrec[:-1])[0] + 1
    return ((mrec[ids] - mrec[ids - 1]) * mpre[ids]).sum() * 10


def average_precision(y_true, y_score):
    """sklearn.metrics.average_precision_score for binary labels: sum over the distinct score thresholds, from the highest score
    down, of (recall_n - recall_{n-1}) * precision_n.  Equal scores share one threshold.  No positive label: recall is taken as 1
    at every threshold (sklearn's convention), which gives the precision at the lowest threshold."""
    y_true = np.asarray(y_true).astype(np.float64)
    y_score = np.asarray(y_score, dtype=np.float64)
    if y_true.size == 0:
        return np.nan
    order = np.argsort(y_score, kind='mergesort')[::-1]
    y_true, y_score = y_true[order], y_score[order]
    ends = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true)[ends]
    fps = 1 + ends - tps
    precision = tps / (tps + fps)
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    precision = np.hstack((precision[::-1], 1.))
    recall = np.hstack((recall[::-1], 0.))
    return -np.sum(np.diff(recall) * precision[:-1])


# ---- grouping and filtering (meters/utils.py:21-96) ---------------------------------------------------------------------------
def add_inst_num(infos, group_keys=GROUP_KEYS, key='pred_inst_num'):
    """number the rows of every group 0, 1, ... in row order"""
    infos[key] = infos.groupby(list(group_keys)).cumcount().values.astype(int) if len(infos) else np.empty(0, dtype=int)
    return infos


def get_top_n_ids(infos, group_keys=GROUP_KEYS, top_key='score', n_top=-1, targets=None):
    """row ids of the n best rows (by top_key, descending) of every group, groups in key order.  n = n_top where positive, else the
    group's `inst_count` in `targets` (0 for a group that is no target), else all rows."""
    group_keys = list(group_keys)
    if len(infos) == 0:
        return []
    order = infos.sort_values(group_keys + [top_key], ascending=[True] * len(group_keys) + [False], kind='stable')
    rank = order.groupby(group_keys).cumcount().values
    if n_top > 0:
        limit = np.full(len(order), n_top)
    elif targets is not None:
        counts = targets.drop_duplicates(group_keys)[group_keys + ['inst_count']]
        limit = order[group_keys].merge(counts, on=group_keys, how='left')['inst_count'].fillna(0).values
    else:
        return order.index.values.copy()
    return order.index.values[rank < limit]


def add_valid_gt(gt_infos, group_keys=GROUP_KEYS, visib_gt_min=-1, targets=None):
    """the `valid` column: visible enough (visib_gt_min > 0, and of a target label), else the most visible inst_count instances of
    every target group, else everything"""
    if visib_gt_min > 0:
        valid = (gt_infos['visib_fract'] >= visib_gt_min).values
        if targets is not None:
            valid = np.logical_and(valid, np.isin(gt_infos['label'], targets['label']))
        gt_infos['valid'] = valid
    elif targets is not None:
        valid = np.zeros(len(gt_infos), dtype=bool)
        valid[np.asarray(get_top_n_ids(gt_infos, group_keys=group_keys, top_key='visib_fract', targets=targets), dtype=int)] = True
        gt_infos['valid'] = valid
    else:
        gt_infos['valid'] = True
    return gt_infos


def get_candidate_matches(pred_infos, gt_infos, group_keys=GROUP_KEYS, only_valids=True):
    """every (prediction, ground truth) pair of one group: predictions in row order, the ground truths of each in row order"""
    pred_infos['pred_id'] = np.arange(len(pred_infos))
    gt_infos['gt_id'] = np.arange(len(gt_infos))
    cand_infos = pred_infos.merge(gt_infos, on=list(group_keys))
    if only_valids:
        cand_infos = cand_infos[cand_infos['valid']].reset_index(drop=True)
    cand_infos['cand_id'] = np.arange(len(cand_infos))
    return cand_infos


def match_poses(cand_infos, group_keys=GROUP_KEYS):
    """Greedy matching inside every group (meters/utils.py:99-129): predictions from the highest score down, each takes the
    candidate of smallest error (the first of equal ones) whose ground truth is still free.  -> the matched rows of cand_infos,
    groups in key order.  Arrays per group; no row-by-row frame access."""
    assert 'error' in cand_infos
    if len(cand_infos) == 0:
        return cand_infos
    gid = cand_infos.groupby(list(group_keys), sort=True).ngroup().values
    pred, gt = cand_infos['pred_id'].values, cand_infos['gt_id'].values
    err, score = cand_infos['error'].values.astype(np.float64), cand_infos['score'].values
    rows_by_group = np.argsort(gid, kind='stable')
    bounds = np.flatnonzero(np.diff(gid[rows_by_group])) + 1
    taken = []
    for rows in np.split(rows_by_group, bounds):
        _, first, inverse = np.unique(pred[rows], return_index=True, return_inverse=True)
        appearance = np.argsort(first, kind='stable')                       # predictions in the order they first appear
        by_score = appearance[np.argsort(-score[rows][first[appearance]], kind='stable')]
        gt_free = {g: True for g in gt[rows]}
        for u in by_score:
            mine = rows[inverse == u]
            e = np.where([gt_free[g] for g in gt[mine]], err[mine], np.inf)
            e[np.isnan(e)] = np.inf
            k = int(np.argmin(e))
            if e[k] < np.inf:
                gt_free[gt[mine[k]]] = False
                taken.append(mine[k])
    return cand_infos.iloc[np.asarray(taken, dtype=int)].reset_index(drop=True)


# ---- the host half of `add` -----------------------------------------------------------------------------------------------------
def prepare_candidates(pred_infos, gt_infos, targets=None, n_top=-1, visib_gt_min=-1, consider_all_predictions=False):
    """pose_meters.py:117-153 on the info frames alone.  -> dict:
      keep_ids       rows of the given predictions that lie in a (scene, view) of the ground truth, in the order the tables use;
      pred_infos     their frame (with pred_inst_id);      filtered_ids   the rows of it that pass the top-n filter, in group order;
      pred_infos_filtered  that selection (pred_id = its row number);      gt_infos  with gt_inst_id, valid, gt_id;
      cand_infos     the tentative pairs (pred_id into the filtered predictions, gt_id into the ground truth)."""
    gt_views = gt_infos.loc[:, ['scene_id', 'view_id']].drop_duplicates().reset_index(drop=True)
    if targets is not None:
        targets = gt_views.merge(targets)
    pred_infos = pred_infos.reset_index(drop=True).copy()
    pred_infos['batch_pred_id'] = np.arange(len(pred_infos))
    keep_ids = gt_views.merge(pred_infos)['batch_pred_id'].values
    pred_infos = pred_infos.iloc[keep_ids].reset_index(drop=True)
    gt_infos = gt_infos.reset_index(drop=True).copy()
    pred_infos = add_inst_num(pred_infos, key='pred_inst_id')
    gt_infos = add_inst_num(gt_infos, key='gt_inst_id')
    if not consider_all_predictions:
        filtered_ids = np.asarray(get_top_n_ids(pred_infos, top_key='score', targets=targets, n_top=n_top), dtype=int)
    else:
        filtered_ids = np.arange(len(pred_infos))
    pred_infos_filtered = pred_infos.iloc[filtered_ids].reset_index(drop=True)
    gt_infos = add_valid_gt(gt_infos, targets=targets, visib_gt_min=visib_gt_min)
    cand_infos = get_candidate_matches(pred_infos_filtered, gt_infos, only_valids=True)
    return dict(keep_ids=keep_ids, pred_infos=pred_infos, filtered_ids=filtered_ids, pred_infos_filtered=pred_infos_filtered,
                gt_infos=gt_infos, cand_infos=cand_infos)


def spheres_overlap_filter(cand_infos, t_pred, t_gt, diameters):
    """keep the pairs whose centres are closer than the object's diameter (float32, as the reference compares them)"""
    d = np.asarray(t_pred, dtype=np.float32) - np.asarray(t_gt, dtype=np.float32)
    norm = np.sqrt((d * d).sum(-1, dtype=np.float32)) if len(d) else np.zeros(0, np.float32)
    keep = np.where(norm < np.asarray(diameters, dtype=np.float32))[0]
    cand_infos = cand_infos.iloc[keep].reset_index(drop=True)
    cand_infos['cand_id'] = np.arange(len(cand_infos))
    return cand_infos


def _vector_column(array):
    col = np.empty(len(array), dtype=object)
    for n in range(len(array)):
        col[n] = array[n]
    return col


def _left_fill(left, right, on, names, fill_values=FILL_VALUES):
    """xr_merge (utils/xarray.py:4-42) for frames: the columns `names` of `right` brought to the rows of `left` that share `on` (at
    most one row of `right` each), the other rows filled by fill_values; dtypes as the reference's: that of the fill value."""
    idx = left[on].merge(right[on].assign(_idx2=np.arange(len(right))), on=on, how='left')['_idx2'].values.astype(np.float64)
    assert len(idx) == len(left), 'more than one match for a row'
    has = np.isfinite(idx)
    src = idx[has].astype(int)
    out = {}
    for k in names:
        fill = fill_values.get(k, float('nan'))
        if k in VECTOR_SHAPES:
            arr = np.empty((len(left),) + VECTOR_SHAPES[k], dtype=np.array(fill).dtype)
            arr[:] = fill
            if len(src):
                arr[has] = np.stack(list(right[k].values[src]))
            out[k] = _vector_column(arr)
        else:
            arr = np.empty(len(left), dtype=np.array(fill).dtype)
            arr[:] = fill
            arr[has] = right[k].values[src]
            out[k] = arr
    return out


def match_tables(cand_infos, errors, pred_infos, gt_infos, diameters, match_threshold=0.1, pred_poses=None):
    """pose_meters.py:174-228 on the host.  cand_infos: the tentative pairs (after the sphere filter), errors: dict of numpy arrays
    indexed by cand_id (norm_avg (n), xyz_avg (n,3), TCO_xyz (n,3), TCO_norm (n)), pred_infos / gt_infos: prepare_candidates',
    diameters: {label: diameter_m}, pred_poses (n_pred,4,4) optional (NaN when absent).
    -> (matches, gt, preds) frames, (kept cand_infos) as a fourth value."""
    on_pred, on_gt = GROUP_KEYS + ['pred_inst_id'], GROUP_KEYS + ['gt_inst_id']
    norm_avg = np.asarray(errors['norm_avg'])
    cand_infos = cand_infos.copy()
    cand_infos['error'] = norm_avg
    cand_infos['obj_diameter'] = np.array([diameters[k] for k in cand_infos['label']], dtype=np.float64)
    keep = cand_infos['error'] <= match_threshold * cand_infos['obj_diameter']
    cand_infos = cand_infos[keep].reset_index(drop=True)
    matched = match_poses(cand_infos)

    gt = gt_infos.loc[:, GROUP_KEYS + ['gt_inst_id', 'valid']].reset_index(drop=True).copy()     # (the reference never keeps visib_fract)
    preds = pred_infos.loc[:, GROUP_KEYS + ['pred_inst_id', 'score']].reset_index(drop=True).copy()
    matches = matched.loc[:, GROUP_KEYS + ['pred_inst_id', 'gt_inst_id', 'cand_id']].reset_index(drop=True).copy()
    cand = matches['cand_id'].values.astype(int)
    matches['obj_diameter'] = np.array([diameters[k] for k in matches['label']], dtype=np.float64)
    matches['norm'] = norm_avg[cand]
    matches['0.1d'] = matches['norm'].values < 0.1 * matches['obj_diameter'].values
    matches['xyz'] = _vector_column(np.asarray(errors['xyz_avg'])[cand])
    matches['TCO_xyz'] = _vector_column(np.asarray(errors['TCO_xyz'])[cand])
    matches['TCO_norm'] = np.asarray(errors['TCO_norm'])[cand]
    poses = np.full((len(preds), 4, 4), np.nan, dtype=np.float32) if pred_poses is None else np.asarray(pred_poses)
    preds['TXO_pred'] = _vector_column(poses)

    for k, v in _left_fill(matches, preds, on_pred, ['score', 'TXO_pred']).items():
        matches[k] = v
    from_matches = ['pred_inst_id', 'cand_id', 'obj_diameter', 'norm', '0.1d', 'xyz', 'TCO_xyz', 'TCO_norm', 'score', 'TXO_pred']
    for k, v in _left_fill(gt, matches, on_gt, from_matches).items():
        gt[k] = v
    preds['0.1d'] = _left_fill(preds, matches, on_pred, ['0.1d'])['0.1d']
    return matches, gt, preds, cand_infos


# ---- summary (pose_meters.py:230-322) -----------------------------------------------------------------------------------------------
def _mean_rows(column, shape):
    if len(column) == 0:
        return np.full(shape, np.nan).tolist()
    return np.stack(list(column)).astype(np.float64).mean(0).tolist()


def summarize(gt_df, matches_df, pred_df, n_top=-1, report_AP=False, report_error_AUC=False, report_error_stats=False):
    """-> (summary dict, dict of frames / values): see PoseErrorMeter.summary"""
    valid_df = gt_df[gt_df['valid'].values.astype(bool)].reset_index(drop=True)
    AUC = OrderedDict()
    for label in np.unique(valid_df['label'].values) if len(valid_df) else []:
        errors = valid_df['norm'].values[(valid_df['label'] == label).values]
        assert np.all(~np.isnan(errors))
        AUC[label] = compute_auc_posecnn(errors)
    auc_values = np.array(list(AUC.values()), dtype=np.float64)
    auc_mean = np.nan if np.all(np.isnan(auc_values)) else float(np.nanmean(auc_values))     # NaN (no error below 0.1) is skipped, as xarray's mean does
    auc_all = compute_auc_posecnn(valid_df['norm'].values)

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
        label_df['n_tp'] = np.cumsum(label_df['0.1d'].values.astype(float))
        label_df['prec'] = label_df['n_tp'] / (np.arange(len(label_df)) + 1)
        label_df['recall'] = label_df['n_tp'] / label_n_gt
        y_true = label_df['0.1d']
        ap = average_precision(y_true, label_df['score']) * y_true.sum() / label_n_gt
        label_df['AP'] = ap
        label_df['n_gt'] = label_n_gt
        return ap, label_df

    ap_dfs = dict()
    df = pred_df[['label', '0.1d', 'score']]
    for label, label_n_gt in n_gts.items():
        label_df = df[(df['label'] == label).values]
        if len(label_df) and label_df['0.1d'].sum() > 0:
            ap_dfs[label] = compute_ap(label_df, label_n_gt)[1]
    if len(ap_dfs) > 0:      # (a label without a single true positive is left out of the mean, not counted as 0)
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
        '0.1d': int(valid_df['0.1d'].sum()) / n_gt_valid,
    }
    if report_error_stats:
        summary.update({
            'norm': float(matches_df['norm'].values.astype(np.float64).mean()) if n_matched else np.nan,
            'xyz': _mean_rows(matches_df['xyz'].values, (3,)),
            'TCO_xyz': _mean_rows(matches_df['TCO_xyz'].values, (3,)),
            'TCO_norm': float(matches_df['TCO_norm'].values.astype(np.float64).mean()) if n_matched else np.nan,
        })
    if report_AP:
        summary.update({'AP': AP, 'mAP': mAP})
    if report_error_AUC:
        summary.update({'AUC/objects/mean': auc_mean, 'AUC': auc_all})
    dfs = dict(gt=gt_df, matches=matches_df, preds=pred_df, ap=ap_dfs, auc_objects=AUC)
    return summary, dfs


# ---- the meter ------------------------------------------------------------------------------------------------------------------------
class PoseErrorMeter:
    """The reference's PoseErrorMeter on a cosypose_amd BatchedMeshes whose infos hold n_points, is_symmetric and diameter_m per
    label.  exact_meshes=True measures every object on its own n_points points; False on point_table(sample_n_points), or on the
    full padded table.  errors_bsz is accepted and ignored: all pairs go in one launch."""

    def __init__(self, mesh_db, error_type='ADD', report_AP=False, report_error_AUC=False, report_error_stats=False,
                 sample_n_points=None, errors_bsz=1, match_threshold=0.1, exact_meshes=True, spheres_overlap_check=True,
                 consider_all_predictions=False, targets=None, visib_gt_min=-1, n_top=-1):
        self.mesh_db = mesh_db
        self.error_type = error_type.upper()
        if self.error_type not in ('ADD', 'ADD-S', 'ADD(-S)'):
            raise ValueError('Error not supported', error_type)
        self.sample_n_points = sample_n_points
        self.errors_bsz = errors_bsz
        self.n_top = n_top
        self.exact_meshes = exact_meshes
        self.visib_gt_min = visib_gt_min
        self.targets = targets
        self.match_threshold = match_threshold
        self.spheres_overlap_check = spheres_overlap_check
        self.consider_all_predictions = consider_all_predictions
        self.report_AP = report_AP
        self.report_error_stats = report_error_stats
        self.report_error_AUC = report_error_AUC
        if exact_meshes:
            assert sample_n_points is None
        self.reset()

    def reset(self):
        self.datas = defaultdict(list)

    def is_data_valid(self, data):
        return hasattr(data, 'poses') and all(k in data.infos for k in GROUP_KEYS)

    # -- device half
    def _points(self):
        """(point table, points used per object)"""
        labels = list(self.mesh_db.labels)
        if self.exact_meshes:
            table = self.mesh_db.points.float().contiguous()
            n_points = np.array([self.mesh_db.infos[l]['n_points'] for l in labels], dtype=np.int32)
        else:
            table = self.mesh_db.point_table(self.sample_n_points) if self.sample_n_points is not None else self.mesh_db.points.float().contiguous()
            n_points = np.full(len(labels), table.shape[1], dtype=np.int32)
        return table, n_points

    def compute_errors(self, TXO_pred, TXO_gt, labels):
        """errors of len(labels) pairs -> dict of device tensors (distances.pose_errors)"""
        from .distances import pose_errors
        table, n_points = self._points()
        infos = self.mesh_db.infos
        if self.error_type == 'ADD(-S)':
            modes = np.array([1 if infos[l]['is_symmetric'] else 0 for l in labels], dtype=np.int32)
        else:
            modes = np.full(len(labels), 1 if self.error_type == 'ADD-S' else 0, dtype=np.int32)
        obj_ids = np.array([self.mesh_db.label_to_id[l] for l in labels], dtype=np.int32)
        return pose_errors(TXO_pred.to(table.device), TXO_gt.to(table.device), obj_ids, modes, table, n_points)

    def add(self, pred_data, gt_data):
        pred_poses_all = pred_data.poses.float()
        gt_poses = gt_data.poses.float()
        prep = prepare_candidates(pred_data.infos, gt_data.infos, targets=self.targets, n_top=self.n_top, visib_gt_min=self.visib_gt_min,
                                  consider_all_predictions=self.consider_all_predictions)
        cand_infos = prep['cand_infos']
        diameters = {l: self.mesh_db.infos[l]['diameter_m'] for l in self.mesh_db.labels}
        pred_poses = pred_poses_all[torch.as_tensor(prep['keep_ids'], dtype=torch.long)]
        filtered_poses = pred_poses[torch.as_tensor(prep['filtered_ids'], dtype=torch.long)]
        if self.spheres_overlap_check:
            t_pred = filtered_poses.cpu().numpy()[cand_infos['pred_id'].values, :3, 3]
            t_gt = gt_poses.cpu().numpy()[cand_infos['gt_id'].values, :3, 3]
            cand_infos = spheres_overlap_filter(cand_infos, t_pred, t_gt, [diameters[k] for k in cand_infos['label']])
        pred_ids = torch.as_tensor(cand_infos['pred_id'].values, dtype=torch.long)
        gt_ids = torch.as_tensor(cand_infos['gt_id'].values, dtype=torch.long)
        errors = self.compute_errors(filtered_poses[pred_ids], gt_poses[gt_ids], cand_infos['label'].values)
        errors = {k: v.cpu().numpy() for k, v in errors.items()}
        matches, gt, preds, kept = match_tables(cand_infos, errors, prep['pred_infos'], prep['gt_infos'], diameters,
                                             match_threshold=self.match_threshold, pred_poses=pred_poses.cpu().numpy())
        self.last_candidates = dict(cand_infos=cand_infos, kept=kept, errors=errors)      # of this `add`, for inspection
        self.datas['gt_df'].append(gt)
        self.datas['pred_df'].append(preds)
        self.datas['matches_df'].append(matches)

    def summary(self):
        gt_df = pd.concat(self.datas['gt_df'], axis=0, ignore_index=True)
        matches_df = pd.concat(self.datas['matches_df'], axis=0, ignore_index=True)
        pred_df = pd.concat(self.datas['pred_df'], axis=0, ignore_index=True)
        return summarize(gt_df, matches_df, pred_df, n_top=self.n_top, report_AP=self.report_AP, report_error_AUC=self.report_error_AUC,
                         report_error_stats=self.report_error_stats)

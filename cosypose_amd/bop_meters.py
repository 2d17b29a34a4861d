"""BOP-2020 scores: the recall of MSSD, MSPD and VSD over their threshold settings and AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3, the
number the BOP leaderboard ranks on (Hodan et al., "BOP Challenge 2020", section 2.4).  The reference writes a CSV and starts the BOP
toolkit for these (scripts/run_bop_eval.py:58-70, run_bop20_eval.py); the toolkit is not part of the reference checkout, so the
contract is the published definition, restated in DESIGN.md section 15 and as a numpy twin in tests/bop_ref.py -- not a recording.

What runs where
  * device: ONE bop_errors call for all tentative (prediction, ground truth) pairs of an `add`;
  * host, numpy in float64: grouping and filtering (pose_meters.prepare_candidates), the greedy matching per (scene, view, label) group
    and threshold setting (match_counts) and everything `summary` reports.
match_counts takes tables alone, so the host half runs (and is tested) without a device.
"""
from collections import OrderedDict

import numpy as np
import pandas as pd
import torch

from .bop_errors import VSD_DELTA, VSD_TAUS, VSD_THRESHOLDS, MSSD_THRESHOLDS, MSPD_THRESHOLDS
from .pose_meters import GROUP_KEYS, prepare_candidates


def match_counts(group, pred_row, gt_row, score, n_valid, err, theta):
    """Greedy matching of one `add`, all threshold settings at once.
    group (n_cand,) group number of every tentative pair, pred_row / gt_row (n_cand,) the pair's prediction and ground truth (row
    numbers: the lower row wins a tie), score (n_cand,) the prediction's score, n_valid {group: valid ground-truth instances},
    err (n_cand, n_set) float64 and theta (n_cand, n_set) the error and its threshold under every setting.
    Per group and setting: predictions in descending score (ties: lower row), the first n_valid[group] of them only; each takes,
    among the group's ground truths that are still free and have err < theta, the one of smallest error (ties: lower row).
    -> {group: (n_set,) int64 number of matched ground truths}"""
    group, pred_row, gt_row = np.asarray(group), np.asarray(pred_row), np.asarray(gt_row)
    score = np.asarray(score, dtype=np.float64)
    err, theta = np.asarray(err, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    n_set = err.shape[1]
    out = {}
    for g in np.unique(group):
        rows = np.flatnonzero(group == g)
        preds, p_first = np.unique(pred_row[rows], return_index=True)          # ascending row number
        order = preds[np.argsort(-score[rows][p_first], kind='stable')][:int(n_valid.get(g, 0))]
        gts = np.unique(gt_row[rows])
        gt_at = {v: k for k, v in enumerate(gts)}
        free = np.ones((len(gts), n_set), dtype=bool)
        matched = np.zeros(n_set, dtype=np.int64)
        for p in order:
            mine = rows[pred_row[rows] == p]
            e = np.full((len(gts), n_set), np.inf)
            ok = err[mine] < theta[mine]                                        # a NaN error is below no threshold
            at = np.array([gt_at[v] for v in gt_row[mine]], dtype=int)
            e[at] = np.where(ok, err[mine], np.inf)
            e[~free] = np.inf
            k = np.argmin(e, axis=0)                                            # the first minimum: the lower ground-truth row
            took = e[k, np.arange(n_set)] < np.inf
            free[k[took], np.flatnonzero(took)] = False
            matched += took
        out[g] = matched
    return out


def settings_tables(errors, diameters, width, vsd_thresholds=VSD_THRESHOLDS, mssd_thresholds=MSSD_THRESHOLDS, mspd_thresholds=MSPD_THRESHOLDS):
    """(err, theta) of every metric for match_counts.  errors: dict of numpy arrays per tentative pair, vsd (n, n_tau) float64, mssd (n,),
    mspd (n,); diameters (n,) of the pairs' objects; width: the frames' width in pixels.
    vsd: the n_tau x len(vsd_thresholds) settings, tau-major; mssd: theta x diameter; mspd: theta x width / 640."""
    n = len(diameters)
    d = np.asarray(diameters, dtype=np.float64).reshape(n, 1)
    vsd = np.asarray(errors['vsd'], dtype=np.float64)
    assert vsd.shape[:1] == (n,) and vsd.ndim == 2, vsd.shape          # (n, n_tau), also for n = 0: an `add` without a tentative pair
    th_v = np.asarray(vsd_thresholds, dtype=np.float64)
    out = OrderedDict()
    out['vsd'] = (np.repeat(vsd, len(th_v), axis=1), np.tile(th_v, (n, vsd.shape[1])))
    out['mssd'] = (np.repeat(np.asarray(errors['mssd'], dtype=np.float64).reshape(n, 1), len(mssd_thresholds), axis=1),
                   np.asarray(mssd_thresholds, dtype=np.float64)[None, :] * d)
    out['mspd'] = (np.repeat(np.asarray(errors['mspd'], dtype=np.float64).reshape(n, 1), len(mspd_thresholds), axis=1),
                   np.tile(np.asarray(mspd_thresholds, dtype=np.float64) * (width / 640.0), (n, 1)))
    return out


def group_table(cand_infos, gt_infos, errors, diameters, width, **thresholds):
    """The host half of one `add`: -> frame with one row per (scene, view, label) group that has valid ground truth: the group keys,
    n_valid, and matched_vsd / matched_mssd / matched_mspd (object columns: int64 arrays, one entry per setting)."""
    valid = gt_infos[gt_infos['valid'].values.astype(bool)]
    groups = valid.groupby(GROUP_KEYS, sort=True).size().reset_index(name='n_valid')
    key_to_group = {tuple(k): n for n, k in enumerate(groups[GROUP_KEYS].itertuples(index=False, name=None))}
    group = np.array([key_to_group[tuple(k)] for k in cand_infos[GROUP_KEYS].itertuples(index=False, name=None)], dtype=np.int64)
    n_valid = dict(enumerate(groups['n_valid'].values))
    tables = settings_tables(errors, diameters, width, **thresholds)
    for name, (err, theta) in tables.items():
        got = match_counts(group, cand_infos['pred_id'].values, cand_infos['gt_id'].values, cand_infos['score'].values, n_valid, err, theta)
        col = np.empty(len(groups), dtype=object)
        for g in range(len(groups)):
            col[g] = got.get(g, np.zeros(err.shape[1], dtype=np.int64))
        groups['matched_' + name] = col
    return groups


def summarize(groups):
    """recall = matched valid ground truth / valid ground truth over all groups, per setting; AR_x = its mean over the settings of
    metric x; AR = the mean of the three.  The same per label.  -> (summary dict, dict of frames)"""
    def recalls(g):
        n = int(g['n_valid'].sum())
        out = {}
        for name in ('vsd', 'mssd', 'mspd'):
            matched = np.sum(np.stack(list(g['matched_' + name].values)), axis=0) if len(g) else np.zeros(1)
            out[name] = float(np.mean(matched / n)) if n else float('nan')
        return out, n

    r, n = recalls(groups)
    summary = OrderedDict(n_gt_valid=n, AR_VSD=r['vsd'], AR_MSSD=r['mssd'], AR_MSPD=r['mspd'], AR=(r['vsd'] + r['mssd'] + r['mspd']) / 3)
    rows = []
    for label in np.unique(groups['label'].values) if len(groups) else []:
        r, n = recalls(groups[(groups['label'] == label).values])
        rows.append(dict(label=label, n_gt_valid=n, AR_VSD=r['vsd'], AR_MSSD=r['mssd'], AR_MSPD=r['mspd'], AR=(r['vsd'] + r['mssd'] + r['mspd']) / 3))
        for k in ('AR_VSD', 'AR_MSSD', 'AR_MSPD', 'AR'):
            summary[f'{k}/objects/{label}'] = rows[-1][k]
    labels = pd.DataFrame(rows, columns=['label', 'n_gt_valid', 'AR_VSD', 'AR_MSSD', 'AR_MSPD', 'AR'])
    return summary, dict(groups=groups, labels=labels)


class BopScoreMeter:
    """models: BopModels on the device.  taus / delta: VSD's misalignment tolerances (fractions of the diameter) and visibility
    tolerance; *_thresholds: the thresholds of correctness; targets / visib_gt_min / n_top / consider_all_predictions: as
    PoseErrorMeter (which ground truth is valid, which predictions are kept), visib_gt_min defaulting to BOP's 0.1;
    max_workspace_bytes: the cap of bop_errors' window store."""

    def __init__(self, models, taus=VSD_TAUS, delta=VSD_DELTA, vsd_thresholds=VSD_THRESHOLDS, mssd_thresholds=MSSD_THRESHOLDS,
                 mspd_thresholds=MSPD_THRESHOLDS, targets=None, visib_gt_min=0.1, n_top=-1, consider_all_predictions=False,
                 max_workspace_bytes=None):
        self.models = models
        self.taus, self.delta = tuple(taus), float(delta)
        self.thresholds = dict(vsd_thresholds=tuple(vsd_thresholds), mssd_thresholds=tuple(mssd_thresholds), mspd_thresholds=tuple(mspd_thresholds))
        self.targets, self.visib_gt_min, self.n_top = targets, visib_gt_min, n_top
        self.consider_all_predictions = consider_all_predictions
        self.max_workspace_bytes = max_workspace_bytes
        self.reset()

    def reset(self):
        self.datas = dict(groups=[], n_gt=0, n_pred=0)

    def is_data_valid(self, data):
        return hasattr(data, 'poses') and all(k in data.infos for k in GROUP_KEYS)

    def add(self, pred_data, gt_data, cameras, depth):
        """pred_data / gt_data: collections with `poses` (TCO) and infos scene_id, view_id, label (+ score / visib_fract); cameras:
        collection with `K` and infos scene_id, view_id, one row per view; depth (len(cameras),H,W) measured depth in metres, 0 =
        missing, rows as cameras."""
        from .bop_errors import bop_errors
        models = self.models
        prep = prepare_candidates(pred_data.infos, gt_data.infos, targets=self.targets, n_top=self.n_top, visib_gt_min=self.visib_gt_min,
                                  consider_all_predictions=self.consider_all_predictions)
        cand = prep['cand_infos']
        pred_poses = pred_data.poses.float()[torch.as_tensor(prep['keep_ids'], dtype=torch.long)]
        pred_poses = pred_poses[torch.as_tensor(prep['filtered_ids'], dtype=torch.long)]
        gt_poses = gt_data.poses.float()
        cam_row = {tuple(k): n for n, k in enumerate(cameras.infos[['scene_id', 'view_id']].itertuples(index=False, name=None))}
        try:
            view_ids = np.array([cam_row[tuple(k)] for k in cand[['scene_id', 'view_id']].itertuples(index=False, name=None)], dtype=np.int32)
        except KeyError as e:
            raise ValueError(f'no camera for (scene_id, view_id) = {e.args[0]}') from None
        obj_ids = np.array([models.label_to_id[l] for l in cand['label'].values], dtype=np.int32)
        dev = models.meshes.verts.device
        errors = bop_errors(pred_poses[torch.as_tensor(cand['pred_id'].values, dtype=torch.long)].to(dev),
                            gt_poses[torch.as_tensor(cand['gt_id'].values, dtype=torch.long)].to(dev), obj_ids, view_ids, cameras.K.to(dev),
                            depth.to(dev), models, taus=self.taus, delta=self.delta, max_workspace_bytes=self.max_workspace_bytes)
        errors = {k: v.cpu().numpy() for k, v in errors.items()}
        groups = group_table(cand, prep['gt_infos'], errors, models.diameters[obj_ids], depth.shape[-1], **self.thresholds)
        self.last_candidates = dict(cand_infos=cand, errors=errors, view_ids=view_ids, obj_ids=obj_ids)      # of this `add`, for inspection
        self.datas['groups'].append(groups)
        self.datas['n_gt'] += len(prep['gt_infos'])
        self.datas['n_pred'] += len(prep['pred_infos'])

    def summary(self):
        groups = pd.concat(self.datas['groups'], axis=0, ignore_index=True)
        summary, dfs = summarize(groups)
        summary.update(n_gt=self.datas['n_gt'], n_pred=self.datas['n_pred'])
        return summary, dfs

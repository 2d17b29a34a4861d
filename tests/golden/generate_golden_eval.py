#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_eval.npz: the REFERENCE's pose meter (cosypose/evaluation/meters/pose_meters.py with
meters/utils.py, run in place on the CPU, one thread) on seeded synthetic scenes (cosypose_amd.synthetic.make_eval_meshes /
make_eval_scene).  Run in the build container only:   python tests/golden/generate_golden_eval.py

Shims, next to generate_golden.install_stubs (import stubs, path of the reference):
  * np.int = int, np.float = float      (meters/utils.py:25, pose_meters.py:266 use the aliases numpy dropped);
  * an EMPTY module named xarray        (pose_meters.py:3 imports it; it is not installed here);
  * torch.Tensor.cuda = identity, torch.set_num_threads(1).

What runs as the reference wrote it, in the order `add` and `summary` call it:
  PoseErrorMeter.compute_errors_batch / compute_errors (pose_meters.py:53-114, with lib3d/distances.py and the reference's own
  BatchedMeshes), add_inst_num, get_top_n_ids, add_valid_gt, get_candidate_matches, match_poses, compute_auc_posecnn
  (meters/utils.py) and sklearn's average_precision_score.
What CANNOT run here and is RESTATED below, because it goes through xarray: the three xr_merge calls and the variables added to
the datasets (pose_meters.py:183-228 -> tables()), and the group-bys, means and selections of `summary` (:230-322 -> summarize()).
The lines of `add` between the calls above (:117-181: frame selections, the sphere test, the threshold) are pandas / torch
one-liners and are restated with them, line for line (reference_add()).  xarray's mean skips NaN for float data; that is how
'AUC/objects/mean' is taken here.  The float32 means of report_error_stats are taken in float64.

The fixture holds ids, poses, scores, the recorded tables and summaries; meshes are regenerated from MESH_SEED by the tests.

The generator ASSERTS what lets the tests compare everything, with no case left out (if a seed violates one, change the seed, not
the bound): scores are all different; no candidate's error is within 1e-3 (relative) of match_threshold * d, of 0.1 * d or of the
AUC cut-off 0.1; no centre distance within 1e-3 of the diameter; no two candidates of one prediction have errors within 1e-3 of
each other; and the whole pipeline run in float32 and in float64 gives the same tables.  It also records, per error field, the
largest relative deviation between the reference in float32 and in float64.
"""
import sys
import types
import pathlib
import warnings

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import numpy as np
import pandas as pd
import torch

import generate_golden as gg
from generate_golden_ba import save_npz
from cosypose_amd import synthetic as syn

MESH_SEED = 501
SCENE_SEED = 512
SCENE_IDS = (3, 7)            # one `add` per scene, one `summary` over both
GROUP_KEYS = ['scene_id', 'view_id', 'label']
CONFIGS = {
    'add': dict(error_type='ADD'),
    'adds': dict(error_type='ADD-S'),
    'addms': dict(error_type='ADD(-S)'),
    'addms_sampled': dict(error_type='ADD(-S)', exact_meshes=False, sample_n_points=100),
    'adds_padded': dict(error_type='ADD-S', exact_meshes=False),
    'addms_ntop': dict(error_type='ADD(-S)', n_top=1),
    'addms_targets': dict(error_type='ADD(-S)', targets=True),
    'add_visib': dict(error_type='ADD', targets=True, visib_gt_min=0.3),
    'addms_all': dict(error_type='ADD(-S)', consider_all_predictions=True),
    'addms_nosphere': dict(error_type='ADD(-S)', spheres_overlap_check=False),
    'addms_loose': dict(error_type='ADD(-S)', match_threshold=0.45),
}
DEFAULTS = dict(match_threshold=0.1, exact_meshes=True, sample_n_points=None, spheres_overlap_check=True, consider_all_predictions=False,
                targets=False, visib_gt_min=-1, n_top=-1)
MARGIN = 1e-3
ERROR_FIELDS = ('norm_avg', 'xyz_avg', 'TCO_xyz', 'TCO_norm')


def reference():
    gg.install_stubs()
    np.int = int
    np.float = float
    sys.modules['xarray'] = types.ModuleType('xarray')
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_num_threads(1)
    from cosypose.lib3d.rigid_mesh_database import BatchedMeshes
    from cosypose.evaluation.meters import pose_meters, utils
    from sklearn.metrics import average_precision_score
    return dict(BatchedMeshes=BatchedMeshes, PoseErrorMeter=pose_meters.PoseErrorMeter, utils=utils, ap=average_precision_score)


def make_targets(scene, labels):
    """BOP-style targets: every (scene, view, label) group of the ground truth except the first label's, asking for one instance
    fewer than there are (at least one)"""
    gt = pd.DataFrame(dict(scene_id=scene['gt_scene_id'], view_id=scene['gt_view_id'], label=scene['gt_label']))
    counts = gt.groupby(GROUP_KEYS).size().reset_index(name='n')
    counts = counts[counts['label'] != 0].reset_index(drop=True)
    counts['inst_count'] = np.maximum(1, counts['n'] - 1)
    return counts[GROUP_KEYS + ['inst_count']]


def frames(scene, labels, scene_id):
    gsel, psel = scene['gt_scene_id'] == scene_id, scene['pred_scene_id'] == scene_id
    names = np.asarray(labels)
    gt = pd.DataFrame(dict(scene_id=scene['gt_scene_id'][gsel], view_id=scene['gt_view_id'][gsel], label=names[scene['gt_label'][gsel]],
                           visib_fract=scene['gt_visib_fract'][gsel]))
    pred = pd.DataFrame(dict(scene_id=scene['pred_scene_id'][psel], view_id=scene['pred_view_id'][psel],
                             label=names[scene['pred_label'][psel]], score=scene['pred_score'][psel]))
    return gt, scene['gt_poses'][gsel], pred, scene['pred_poses'][psel]


def make_meter(ref, mesh_db, cfg):
    """the reference's meter without its constructor (which moves the meshes to a CUDA device)"""
    m = object.__new__(ref['PoseErrorMeter'])
    m.mesh_db = mesh_db
    m.error_type = cfg['error_type'].upper()
    m.errors_bsz = 1
    m.exact_meshes = cfg['exact_meshes']
    m.sample_n_points = cfg['sample_n_points']
    return m


def reference_add(ref, meter, cfg, infos, targets, gt_infos, gt_poses, pred_infos, pred_poses, dtype):
    """PoseErrorMeter.add up to the matches (pose_meters.py:117-181); every function call is the reference's own"""
    U = ref['utils']
    rec = {}
    gt_infos, pred_infos = gt_infos.copy(), pred_infos.copy()
    gt_poses, pred_poses = torch.as_tensor(gt_poses).to(dtype), torch.as_tensor(pred_poses).to(dtype)
    gt_views = gt_infos.loc[:, ['scene_id', 'view_id']].drop_duplicates().reset_index(drop=True)
    if targets is not None:
        targets = gt_views.merge(targets)
    pred_infos['batch_pred_id'] = np.arange(len(pred_infos))
    keep_ids = gt_views.merge(pred_infos)['batch_pred_id'].values
    pred_infos, pred_poses = pred_infos.iloc[keep_ids].reset_index(drop=True), pred_poses[keep_ids]
    rec['keep_ids'] = keep_ids
    pred_infos = U.add_inst_num(pred_infos, key='pred_inst_id', group_keys=GROUP_KEYS)
    gt_infos = U.add_inst_num(gt_infos, key='gt_inst_id', group_keys=GROUP_KEYS)
    if not cfg['consider_all_predictions']:
        ids = np.asarray(U.get_top_n_ids(pred_infos, group_keys=GROUP_KEYS, top_key='score', targets=targets, n_top=cfg['n_top']), dtype=int)
    else:
        ids = np.arange(len(pred_infos))
    filt_infos, filt_poses = pred_infos.iloc[ids].reset_index(drop=True).copy(), pred_poses[ids]
    rec['filtered_ids'] = ids
    gt_infos = U.add_valid_gt(gt_infos, group_keys=GROUP_KEYS, targets=targets, visib_gt_min=cfg['visib_gt_min'])
    rec['gt_valid'] = gt_infos['valid'].values.astype(bool)
    cand = U.get_candidate_matches(filt_infos, gt_infos, group_keys=GROUP_KEYS, only_valids=True)
    diam = lambda frame: [infos[k]['diameter_m'] for k in frame['label']]
    if cfg['spheres_overlap_check']:
        dists = filt_poses[cand['pred_id'].values.tolist()][:, :3, -1] - gt_poses[cand['gt_id'].values.tolist()][:, :3, -1]
        norms, d = torch.norm(dists, dim=-1), torch.as_tensor(diam(cand)).to(dists.dtype)
        assert ((norms - d).abs() > MARGIN * d).all(), 'a centre distance within the margin of the diameter'
        keep = np.where((norms < d).numpy())[0]
        cand = cand.iloc[keep].reset_index(drop=True)
        cand['cand_id'] = np.arange(len(cand))
    rec['cand_pred_id'], rec['cand_gt_id'] = cand['pred_id'].values, cand['gt_id'].values
    errors = meter.compute_errors_batch(filt_poses[cand['pred_id'].values.tolist()], gt_poses[cand['gt_id'].values.tolist()],
                                        cand['label'].values)
    errors = {k: v.numpy() for k, v in errors.items()}
    cand['error'] = errors['norm_avg']
    cand['obj_diameter'] = diam(cand)
    e, d = cand['error'].values.astype(np.float64), cand['obj_diameter'].values
    for cut, what in ((cfg['match_threshold'] * d, 'match_threshold * d'), (0.1 * d, '0.1 d'), (np.full_like(d, 0.1), 'the AUC cut-off')):
        assert (np.abs(e - cut) > MARGIN * cut).all(), f'an error within the margin of {what}'
    for _, g in cand.groupby('pred_id'):
        ee = np.sort(g['error'].values.astype(np.float64))
        assert (np.diff(ee) > MARGIN * ee[1:]).all(), 'two candidates of one prediction with (nearly) the same error'
    kept = cand[cand['error'] <= cfg['match_threshold'] * cand['obj_diameter']].reset_index(drop=True)
    rec['kept_cand_id'] = kept['cand_id'].values
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        matches = U.match_poses(kept, group_keys=GROUP_KEYS)
    matches = matches.loc[:, GROUP_KEYS + ['pred_inst_id', 'gt_inst_id', 'cand_id']]
    rec['match_cand_id'] = matches['cand_id'].values.astype(int)
    rec['match_pred_id'] = cand['pred_id'].values[rec['match_cand_id']]
    rec['match_gt_id'] = cand['gt_id'].values[rec['match_cand_id']]
    return rec, errors, matches, gt_infos, pred_infos


def tables(infos, errors, matches, gt_infos, pred_infos):
    """RESTATED (xarray): what pose_meters.py:183-228 leaves in the gt / preds / matches datasets, written as plain loops"""
    cid = matches['cand_id'].values.astype(int)
    m = matches.reset_index(drop=True).copy()
    m['obj_diameter'] = [infos[k]['diameter_m'] for k in m['label']]
    m['norm'] = errors['norm_avg'][cid]
    m['0.1d'] = errors['norm_avg'][cid] < 0.1 * m['obj_diameter'].values
    pred_key = {tuple(r): n for n, r in enumerate(pred_infos[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False))}
    m['score'] = [pred_infos['score'].values[pred_key[tuple(r)]] for r in m[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False)]
    by_gt = {tuple(r): n for n, r in enumerate(m[GROUP_KEYS + ['gt_inst_id']].itertuples(index=False))}
    by_pred = {tuple(r): n for n, r in enumerate(m[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False))}
    assert len(by_gt) == len(m) and len(by_pred) == len(m)
    gt = gt_infos.loc[:, GROUP_KEYS + ['gt_inst_id', 'valid']].reset_index(drop=True).copy()
    norm, ok, pid, score = np.full(len(gt), np.inf), np.zeros(len(gt), bool), np.full(len(gt), np.nan), np.full(len(gt), np.nan)
    for n, r in enumerate(gt[GROUP_KEYS + ['gt_inst_id']].itertuples(index=False)):
        k = by_gt.get(tuple(r))
        if k is not None:
            norm[n], ok[n], pid[n], score[n] = m['norm'].values[k], m['0.1d'].values[k], m['pred_inst_id'].values[k], m['score'].values[k]
    gt['norm'], gt['0.1d'], gt['pred_inst_id'], gt['score'] = norm, ok, pid, score
    preds = pred_infos.loc[:, GROUP_KEYS + ['pred_inst_id', 'score']].reset_index(drop=True).copy()
    preds['0.1d'] = [bool(m['0.1d'].values[by_pred[tuple(r)]]) if tuple(r) in by_pred else False
                     for r in preds[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False)]
    m['xyz'], m['TCO_xyz'], m['TCO_norm'] = list(errors['xyz_avg'][cid]), list(errors['TCO_xyz'][cid]), errors['TCO_norm'][cid]
    return m, gt, preds


def summarize(ref, gt_df, matches_df, pred_df, n_top):
    """RESTATED (xarray): pose_meters.py:230-322; compute_auc_posecnn and average_precision_score are the reference's / sklearn's"""
    U, ap_score = ref['utils'], ref['ap']
    valid_df = gt_df[gt_df['valid']].reset_index(drop=True)
    AUC = {}
    for label in sorted(set(valid_df['label'])):
        errors = valid_df['norm'].values[valid_df['label'].values == label]
        AUC[label] = U.compute_auc_posecnn(errors)
    auc = np.array(list(AUC.values()))
    out = {'AUC/objects/mean': np.nanmean(auc) if np.isfinite(auc).any() else np.nan, 'AUC': U.compute_auc_posecnn(valid_df['norm'].values)}
    n_gts = {}
    if n_top > 0:
        subdf = gt_df[GROUP_KEYS + ['valid']].groupby(GROUP_KEYS).sum().reset_index()
        subdf['gt_count'] = np.minimum(n_top, subdf['valid'])
        for label, group in subdf.groupby('label'):
            n_gts[label] = group['gt_count'].sum()
    else:
        for label in sorted(set(gt_df['label'])):
            n_gts[label] = int(gt_df['valid'].values[gt_df['label'].values == label].sum())

    def compute_ap(label_df, label_n_gt):
        label_df = label_df.sort_values('score', ascending=False).reset_index(drop=True)
        y_true, y_score = label_df['0.1d'], label_df['score']
        return ap_score(y_true, y_score) * y_true.sum() / label_n_gt

    aps = {}
    for label, n in n_gts.items():
        label_df = pred_df[pred_df['label'] == label]
        if len(label_df) and label_df['0.1d'].sum() > 0:
            aps[label] = compute_ap(label_df, n)
    if aps:
        out['mAP'] = np.mean(list(aps.values()))
        out['AP'] = compute_ap(pred_df, sum(n_gts.values()))
    else:
        out['AP'], out['mAP'] = 0., 0.
    n_gt_valid = int(sum(n_gts.values()))
    n_matched = len(matches_df)
    out.update({'n_gt': len(gt_df), 'n_gt_valid': n_gt_valid, 'n_pred': len(pred_df), 'n_matched': n_matched,
                'matched_gt_ratio': n_matched / n_gt_valid, 'pred_matched_ratio': len(pred_df) / max(n_matched, 1),
                '0.1d': int(valid_df['0.1d'].sum()) / n_gt_valid,
                'norm': matches_df['norm'].values.astype(np.float64).mean(),
                'xyz': np.stack(list(matches_df['xyz'])).astype(np.float64).mean(0),
                'TCO_xyz': np.stack(list(matches_df['TCO_xyz'])).astype(np.float64).mean(0),
                'TCO_norm': matches_df['TCO_norm'].values.astype(np.float64).mean()})
    out['AP/labels'] = np.array([aps.get(l, np.nan) for l in sorted(n_gts)])
    out['AUC/labels'] = auc
    return out


def run_config(ref, name, cfg, labels, pts, infos, scene, targets, dtype):
    mesh_db = ref['BatchedMeshes'](infos, labels, torch.as_tensor(pts), torch.eye(4).reshape(1, 1, 4, 4).repeat(len(labels), 1, 1, 1)).to(dtype)
    meter = make_meter(ref, mesh_db, cfg)
    out, dfs = {}, dict(gt=[], matches=[], preds=[])
    for a, scene_id in enumerate(SCENE_IDS):
        gt_infos, gt_poses, pred_infos, pred_poses = frames(scene, labels, scene_id)
        rec, errors, matches, gt_i, pred_i = reference_add(ref, meter, cfg, infos, targets if cfg['targets'] else None, gt_infos, gt_poses,
                                                           pred_infos, pred_poses, dtype)
        m, gt, preds = tables(infos, errors, matches, gt_i, pred_i)
        dfs['gt'].append(gt); dfs['matches'].append(m); dfs['preds'].append(preds)
        for k, v in rec.items():
            out[f'{name}/{a}/{k}'] = np.asarray(v)
        for k in ERROR_FIELDS:
            out[f'{name}/{a}/err_{k}'] = errors[k]
        out[f'{name}/{a}/gt_norm'], out[f'{name}/{a}/gt_0.1d'] = gt['norm'].values, gt['0.1d'].values
        out[f'{name}/{a}/gt_pred_inst_id'], out[f'{name}/{a}/gt_score'] = gt['pred_inst_id'].values, gt['score'].values
        out[f'{name}/{a}/gt_inst_id'], out[f'{name}/{a}/pred_inst_id'] = gt['gt_inst_id'].values, preds['pred_inst_id'].values
        out[f'{name}/{a}/preds_0.1d'] = preds['0.1d'].values.astype(bool)
    summary = summarize(ref, *(pd.concat(dfs[k], ignore_index=True) for k in ('gt', 'matches', 'preds')), cfg['n_top'])
    for k, v in summary.items():
        out[f'{name}/summary/{k}'] = np.asarray(v)
    return out


def main():
    ref = reference()
    labels, pts, infos = syn.make_eval_meshes(MESH_SEED)
    scene = syn.make_eval_scene(SCENE_SEED, labels, infos, scene_ids=SCENE_IDS)
    assert len(np.unique(scene['pred_score'])) == len(scene['pred_score']), 'equal scores'
    targets_ids = make_targets(scene, labels)
    targets = targets_ids.copy()
    targets['label'] = np.asarray(labels)[targets['label'].values]
    out = dict(mesh_seed=np.array(MESH_SEED), scene_ids=np.array(SCENE_IDS), config_names=np.array(list(CONFIGS)))
    out.update({k: v for k, v in scene.items()})
    out.update({f'targets_{k}': targets_ids[k].values for k in targets_ids.columns})
    dev = {k: 0. for k in ERROR_FIELDS}
    for name, over in CONFIGS.items():
        cfg = dict(DEFAULTS, **over)
        r32 = run_config(ref, name, cfg, labels, pts, infos, scene, targets, torch.float32)
        r64 = run_config(ref, name, cfg, labels, pts, infos, scene, targets, torch.float64)
        n_match = 0
        for k in r32:
            if '/err_' in k:
                field = k.split('/err_')[1]
                a, b = r32[k].astype(np.float64), r64[k]
                dev[field] = max(dev[field], float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30), initial=0.)))
            elif k.rsplit('/', 1)[1] in ('gt_norm', 'norm', 'xyz', 'TCO_xyz', 'TCO_norm', 'AUC', 'mean', 'AP', 'mAP', 'labels') or '/summary/A' in k:
                assert np.allclose(r32[k], r64[k], rtol=1e-4, atol=0, equal_nan=True), f'{k}: float32 and float64 disagree'
            else:
                assert np.array_equal(r32[k], r64[k], equal_nan=True), f'{k}: float32 and float64 disagree'
            if k.endswith('match_cand_id'):
                n_match += len(r32[k])
        assert n_match > 0, f'{name}: nothing matched'
        for k in ('cfg_' + c for c in ('match_threshold', 'visib_gt_min', 'n_top')):
            out[f'{name}/{k}'] = np.array(cfg[k[4:]])
        out.update(r32)
        s = {k.split('/summary/')[1]: v for k, v in r32.items() if '/summary/' in k and v.ndim == 0}
        print(name, {k: (round(float(v), 4)) for k, v in s.items()}, flush=True)
    for k, v in dev.items():
        out[f'dev/{k}'] = np.array(v)
    print('float32 vs float64 deviation of the reference:', dev)
    path = HERE / 'reference_golden_eval.npz'
    save_npz(path, out)
    print('wrote', path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()

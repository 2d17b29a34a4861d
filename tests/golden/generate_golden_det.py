#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_det.npz: the REFERENCE's detection meter (cosypose/evaluation/meters/detection_meters.py with
meters/utils.py, run in place on the CPU, one thread) on a seeded synthetic scene (cosypose_amd.synthetic.make_det_scene), and the
reference's make_detections_from_segmentation (cosypose/datasets/utils.py:27-40) on the edge masks of tests/det_ref.py.  Run in the
build container only:   python tests/golden/generate_golden_det.py

Shims, next to generate_golden.install_stubs (import stubs, path of the reference):
  * np.int = int, np.float = float      (meters/utils.py, detection_meters.py:168 use the aliases numpy dropped);
  * an EMPTY module named xarray        (detection_meters.py:3 imports it; it is not installed here);
  * torchvision.ops.box_iou of the torchvision stub = torchvision's formula in torch CPU ops, operation by operation
    (torchvision is not installed here): area = (x2 - x1) * (y2 - y1); lt = max, rb = min; wh = (rb - lt).clamp(min=0);
    inter = w * h; iou = inter / (area1[:, None] + area2 - inter);
  * torch.Tensor.cuda = identity, torch.set_num_threads(1).

What runs as the reference wrote it, in the order `add` and `summary` call it: DetectionMeter.compute_metrics_batch (with
compute_metrics: the full matrix of every errors_bsz chunk and its diagonal), add_inst_num, get_top_n_ids, add_valid_gt,
get_candidate_matches, match_poses (meters/utils.py), sklearn's average_precision_score, and make_detections_from_segmentation.
What CANNOT run here and is RESTATED below, because it goes through xarray: the three xr_merge calls and the variables added to the
datasets (detection_meters.py:111-141 -> tables()) and all of `summary` (:143-209 -> summarize(), which also uses Index.contains, a
method pandas removed).  The lines of `add` between the calls above (:57-109: frame selections and the threshold) are pandas
one-liners and are restated with them, line for line (reference_add()).

The fixture holds arrays and label strings only: the scene, the recorded IoUs, tables and summaries, and the boxes of the edge masks.

The generator ASSERTS what lets the tests compare everything, with no case left out (if a seed violates one, change the seed, not
the bound): scores are all different; no IoU within 1e-3 of either threshold (0.5, 0.75); no two candidates of one prediction have
IoUs within 1e-6 of each other; the pipeline run in float32 and in float64 gives the same tables; the last label has no true positive.
It also records what the restated `summary` does without a single valid ground truth (`zero_valid_raises`: ZeroDivisionError).
"""
import sys
import types
import pathlib
import warnings

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import numpy as np
import pandas as pd
import torch

import generate_golden as gg
from generate_golden_ba import save_npz
from cosypose_amd import synthetic as syn
import det_ref

SCENE_SEED = 613
N_LABELS = 6
SCENE_IDS = (3, 7)            # one `add` per scene, one `summary` over both
GROUP_KEYS = ['scene_id', 'view_id', 'label']
CONFIGS = {
    'default': dict(),
    'iou75': dict(iou_threshold=0.75),
    'ntop': dict(n_top=1),
    'targets': dict(targets=True),
    'targets_visib': dict(targets=True, visib_gt_min=0.3),
    'all': dict(consider_all_predictions=True),
}
DEFAULTS = dict(iou_threshold=0.5, consider_all_predictions=False, targets=False, visib_gt_min=-1, n_top=-1)
THRESHOLDS = (0.5, 0.75)
FILL = {'iou': np.nan, 'iou_valid': False, 'score': np.nan}


def reference():
    gg.install_stubs()
    np.int = int
    np.float = float
    sys.modules['xarray'] = types.ModuleType('xarray')
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_num_threads(1)

    def box_area(boxes):
        return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])

    def box_iou(boxes1, boxes2):
        area1, area2 = box_area(boxes1), box_area(boxes2)
        lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
        rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, :, 0] * wh[:, :, 1]
        union = area1[:, None] + area2 - inter
        return inter / union
    sys.modules['torchvision.ops'].box_iou = box_iou
    from cosypose.evaluation.meters import detection_meters, utils
    from cosypose.datasets.utils import make_detections_from_segmentation
    from sklearn.metrics import average_precision_score
    return dict(DetectionMeter=detection_meters.DetectionMeter, utils=utils, ap=average_precision_score,
                make_detections=make_detections_from_segmentation)


def label_names(n=N_LABELS):
    return [f'obj_{k + 1:06d}' for k in range(n)]


def make_targets(scene):
    """BOP-style targets: every (scene, view, label) group of the ground truth except the first label's, asking for one instance
    fewer than there are (at least one)"""
    gt = pd.DataFrame(dict(scene_id=scene['gt_scene_id'], view_id=scene['gt_view_id'], label=scene['gt_label']))
    counts = gt.groupby(GROUP_KEYS).size().reset_index(name='n')
    counts = counts[counts['label'] != 0].reset_index(drop=True)
    counts['inst_count'] = np.maximum(1, counts['n'] - 1)
    return counts[GROUP_KEYS + ['inst_count']]


def frames(scene, scene_id):
    gsel, psel = scene['gt_scene_id'] == scene_id, scene['pred_scene_id'] == scene_id
    names = np.asarray(label_names())
    gt = pd.DataFrame(dict(scene_id=scene['gt_scene_id'][gsel], view_id=scene['gt_view_id'][gsel], label=names[scene['gt_label'][gsel]],
                           visib_fract=scene['gt_visib_fract'][gsel]))
    pred = pd.DataFrame(dict(scene_id=scene['pred_scene_id'][psel], view_id=scene['pred_view_id'][psel],
                             label=names[scene['pred_label'][psel]], score=scene['pred_score'][psel]))
    return gt, scene['gt_bboxes'][gsel], pred, scene['pred_bboxes'][psel]


def reference_add(ref, meter, cfg, targets, gt_infos, gt_boxes, pred_infos, pred_boxes, dtype):
    """DetectionMeter.add up to the matches (detection_meters.py:57-109); every function call is the reference's own"""
    U = ref['utils']
    rec = {}
    gt_infos, pred_infos = gt_infos.copy(), pred_infos.copy()
    gt_boxes, pred_boxes = torch.as_tensor(gt_boxes).to(dtype), torch.as_tensor(pred_boxes).to(dtype)
    gt_views = gt_infos.loc[:, ['scene_id', 'view_id']].drop_duplicates().reset_index(drop=True)
    if targets is not None:
        targets = gt_views.merge(targets)
    pred_infos['batch_pred_id'] = np.arange(len(pred_infos))
    keep_ids = gt_views.merge(pred_infos)['batch_pred_id'].values
    pred_infos, pred_boxes = pred_infos.iloc[keep_ids].reset_index(drop=True), pred_boxes[keep_ids]
    rec['keep_ids'] = keep_ids
    pred_infos = U.add_inst_num(pred_infos, key='pred_inst_id', group_keys=GROUP_KEYS)
    gt_infos = U.add_inst_num(gt_infos, key='gt_inst_id', group_keys=GROUP_KEYS)
    if not cfg['consider_all_predictions']:
        ids = np.asarray(U.get_top_n_ids(pred_infos, group_keys=GROUP_KEYS, top_key='score', targets=targets, n_top=cfg['n_top']), dtype=int)
    else:
        ids = np.arange(len(pred_infos))
    filt_infos, filt_boxes = pred_infos.iloc[ids].reset_index(drop=True).copy(), pred_boxes[ids]
    rec['filtered_ids'] = ids
    gt_infos = U.add_valid_gt(gt_infos, group_keys=GROUP_KEYS, targets=targets, visib_gt_min=cfg['visib_gt_min'])
    rec['gt_valid'] = gt_infos['valid'].values.astype(bool)
    cand = U.get_candidate_matches(filt_infos, gt_infos, group_keys=GROUP_KEYS, only_valids=True)
    rec['cand_pred_id'], rec['cand_gt_id'] = cand['pred_id'].values, cand['gt_id'].values
    metrics = meter.compute_metrics_batch(filt_boxes[cand['pred_id'].values.tolist()], gt_boxes[cand['gt_id'].values.tolist()])
    ious = metrics['iou'].cpu().numpy()
    rec['iou'] = ious
    for thr in THRESHOLDS:
        assert (np.abs(ious.astype(np.float64) - thr) > 1e-3).all(), f'an IoU within 1e-3 of the threshold {thr}'
    cand['iou'] = ious
    for _, g in cand.groupby('pred_id'):
        assert (np.diff(np.sort(g['iou'].values.astype(np.float64))) > 1e-6).all(), 'two candidates of one prediction with (nearly) the same IoU'
    kept = cand[cand['iou'] >= cfg['iou_threshold']].reset_index(drop=True)
    rec['kept_cand_id'] = kept['cand_id'].values
    kept['error'] = - kept['iou']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        matches = U.match_poses(kept, group_keys=GROUP_KEYS)
    matches = matches.loc[:, GROUP_KEYS + ['pred_inst_id', 'gt_inst_id', 'cand_id']]
    rec['match_cand_id'] = matches['cand_id'].values.astype(int)
    return rec, ious, matches, gt_infos, pred_infos


def tables(cfg, ious, matches, gt_infos, pred_infos):
    """RESTATED (xarray): what detection_meters.py:111-141 leaves in the gt / preds / matches datasets, written as plain loops"""
    cid = matches['cand_id'].values.astype(int)
    m = matches.reset_index(drop=True).copy()
    m['iou'] = ious[cid]
    m['iou_valid'] = ious[cid] >= cfg['iou_threshold']
    pred_key = {tuple(r): n for n, r in enumerate(pred_infos[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False))}
    m['score'] = [pred_infos['score'].values[pred_key[tuple(r)]] for r in m[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False)]
    by_gt = {tuple(r): n for n, r in enumerate(m[GROUP_KEYS + ['gt_inst_id']].itertuples(index=False))}
    by_pred = {tuple(r): n for n, r in enumerate(m[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False))}
    assert len(by_gt) == len(m) and len(by_pred) == len(m)
    gt = gt_infos.loc[:, GROUP_KEYS + ['gt_inst_id', 'valid']].reset_index(drop=True).copy()     # (line 112: never visib_fract)
    n = len(gt)
    cols = dict(pred_inst_id=np.full(n, np.nan), cand_id=np.full(n, np.nan), iou=np.full(n, FILL['iou']), iou_valid=np.full(n, FILL['iou_valid']),
                score=np.full(n, FILL['score']))
    for row, r in enumerate(gt[GROUP_KEYS + ['gt_inst_id']].itertuples(index=False)):
        k = by_gt.get(tuple(r))
        if k is not None:
            for name in cols:
                cols[name][row] = m[name].values[k]
    for name, v in cols.items():
        gt[name] = v
    preds = pred_infos.loc[:, GROUP_KEYS + ['pred_inst_id', 'score']].reset_index(drop=True).copy()
    preds['iou_valid'] = [bool(m['iou_valid'].values[by_pred[tuple(r)]]) if tuple(r) in by_pred else FILL['iou_valid']
                          for r in preds[GROUP_KEYS + ['pred_inst_id']].itertuples(index=False)]
    return m, gt, preds


def summarize(ref, gt_df, matches_df, pred_df, n_top):
    """RESTATED (xarray, Index.contains): detection_meters.py:143-209; average_precision_score is sklearn's"""
    ap_score = ref['ap']
    valid_df = gt_df[gt_df['valid']].reset_index(drop=True)
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
        y_true, y_score = label_df['iou_valid'], label_df['score']
        return ap_score(y_true, y_score) * y_true.sum() / label_n_gt

    aps = {}
    for label, n in n_gts.items():
        label_df = pred_df[pred_df['label'] == label]
        if len(label_df) and label_df['iou_valid'].sum() > 0:
            aps[label] = compute_ap(label_df, n)
    out = {}
    if aps:
        out['mAP'] = np.mean(list(aps.values()))
        out['AP'] = compute_ap(pred_df, sum(n_gts.values()))
    else:
        out['AP'], out['mAP'] = 0., 0.
    n_gt_valid = int(sum(n_gts.values()))
    n_matched = len(matches_df)
    out.update({'n_gt': len(gt_df), 'n_gt_valid': n_gt_valid, 'n_pred': len(pred_df), 'n_matched': n_matched,
                'matched_gt_ratio': n_matched / n_gt_valid, 'pred_matched_ratio': len(pred_df) / max(n_matched, 1),
                'iou_valid_recall': int(valid_df['iou_valid'].sum()) / n_gt_valid})
    out['AP/labels'] = np.array([aps.get(l, np.nan) for l in sorted(n_gts)])
    out['n_gt/labels'] = np.array([n_gts[l] for l in sorted(n_gts)])
    out['labels'] = np.array([label_names().index(l) for l in sorted(n_gts)])
    return out


# A table is stored as ONE float64 matrix (columns, rows), columns in this order, `label` as its index into `labels` (integers and
# booleans are exact in float64); the scalar summary values as one vector in SUMMARY_KEYS order.
SUMMARY_KEYS = ('n_gt', 'n_gt_valid', 'n_pred', 'n_matched', 'matched_gt_ratio', 'pred_matched_ratio', 'iou_valid_recall', 'AP', 'mAP')
TABLE_COLUMNS = {'matches': ('scene_id', 'view_id', 'label', 'pred_inst_id', 'gt_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'),
                 'gt': ('scene_id', 'view_id', 'label', 'gt_inst_id', 'valid', 'pred_inst_id', 'cand_id', 'iou', 'iou_valid', 'score'),
                 'preds': ('scene_id', 'view_id', 'label', 'pred_inst_id', 'score', 'iou_valid')}


def run_config(ref, name, cfg, scene, targets, dtype):
    meter = ref['DetectionMeter'](iou_threshold=cfg['iou_threshold'], errors_bsz=16)      # several chunks, the last one ragged
    out, dfs = {}, dict(gt=[], matches=[], preds=[])
    for a, scene_id in enumerate(SCENE_IDS):
        gt_infos, gt_boxes, pred_infos, pred_boxes = frames(scene, scene_id)
        rec, ious, matches, gt_i, pred_i = reference_add(ref, meter, cfg, targets if cfg['targets'] else None, gt_infos, gt_boxes, pred_infos,
                                                         pred_boxes, dtype)
        m, gt, preds = tables(cfg, ious, matches, gt_i, pred_i)
        dfs['gt'].append(gt); dfs['matches'].append(m); dfs['preds'].append(preds)
        for k, v in rec.items():
            out[f'{name}/{a}/{k}'] = np.asarray(v)
        for table, frame in (('matches', m), ('gt', gt), ('preds', preds)):
            assert set(frame.columns) == set(TABLE_COLUMNS[table]), (table, list(frame.columns))
            index = {l: n for n, l in enumerate(label_names())}
            out[f'{name}/{a}/{table}'] = np.stack([np.array([index[l] for l in frame[col]], dtype=np.float64) if col == 'label'
                                                  else frame[col].values.astype(np.float64) for col in TABLE_COLUMNS[table]]).reshape(len(TABLE_COLUMNS[table]), -1)
    cat = {k: pd.concat(dfs[k], ignore_index=True) for k in dfs}
    summary = summarize(ref, cat['gt'], cat['matches'], cat['preds'], cfg['n_top'])
    out[f'{name}/summary'] = np.array([summary[k] for k in SUMMARY_KEYS], dtype=np.float64)
    for k in ('AP/labels', 'n_gt/labels', 'labels'):
        out[f'{name}/summary/{k}'] = np.asarray(summary[k])
    return out, cat


def segmentation_cases(ref):
    """the reference's make_detections_from_segmentation on the uint8 edge masks -> per frame: image, id and box of every detection"""
    out = {}
    for H, W in det_ref.FRAMES:
        masks = det_ref.edge_masks(H, W)
        dets = ref['make_detections'](torch.from_numpy(masks))
        rows = [(b, i, *box.tolist()) for b, d in enumerate(dets) for i, box in d.items()]
        out[f'seg/{H}x{W}'] = np.array(rows, dtype=np.int16).reshape(-1, 6)
        twin = det_ref.detections(masks, 256)
        assert [{i: tuple(box.tolist()) for i, box in d.items()} for d in dets] == twin, f'twin and reference differ at {H}x{W}'
    return out


def main():
    ref = reference()
    scene = syn.make_det_scene(SCENE_SEED, n_labels=N_LABELS, scene_ids=SCENE_IDS)
    assert len(np.unique(scene['pred_score'])) == len(scene['pred_score']), 'equal scores'
    targets_ids = make_targets(scene)
    targets = targets_ids.copy()
    targets['label'] = np.asarray(label_names())[targets['label'].values]
    out = dict(scene_seed=np.array(SCENE_SEED), scene_ids=np.array(SCENE_IDS), config_names=np.array(list(CONFIGS)), labels=np.array(label_names()))
    out.update({k: v for k, v in scene.items()})
    out.update({f'targets_{k}': targets_ids[k].values for k in targets_ids.columns})
    for name, over in CONFIGS.items():
        cfg = dict(DEFAULTS, **over)
        r32, cat = run_config(ref, name, cfg, scene, targets, torch.float32)
        r64, _ = run_config(ref, name, cfg, scene, targets, torch.float64)
        for k in r32:
            if k.endswith('/iou'):
                assert np.allclose(r32[k], r64[k], rtol=1e-5, atol=1e-7, equal_nan=True), f'{k}: float32 and float64 disagree'
            elif k.rsplit('/', 1)[1] in TABLE_COLUMNS:          # the iou row to float32's precision, every other row exactly
                row = TABLE_COLUMNS[k.rsplit('/', 1)[1]].index('iou') if 'iou' in TABLE_COLUMNS[k.rsplit('/', 1)[1]] else None
                exact = [n for n in range(len(r32[k])) if n != row]
                assert np.array_equal(r32[k][exact], r64[k][exact], equal_nan=True), f'{k}: float32 and float64 disagree'
                assert row is None or np.allclose(r32[k][row], r64[k][row], rtol=1e-5, atol=1e-7, equal_nan=True), f'{k}: float32 and float64 disagree'
            elif '/summary' in k and r32[k].dtype.kind == 'f':
                assert np.allclose(r32[k], r64[k], rtol=1e-12, atol=0, equal_nan=True), f'{k}: float32 and float64 disagree'
            else:
                assert np.array_equal(r32[k], r64[k], equal_nan=r32[k].dtype.kind == 'f'), f'{k}: float32 and float64 disagree'
        assert sum(len(v) for k, v in r32.items() if k.endswith('match_cand_id')) > 0, f'{name}: nothing matched'
        last = label_names()[-1]
        assert not cat['preds']['iou_valid'].values[cat['preds']['label'].values == last].any(), 'the last label has a true positive'
        assert (cat['preds']['label'].values == last).any() and (cat['gt']['label'].values == last).any()
        for k in ('iou_threshold', 'visib_gt_min', 'n_top', 'consider_all_predictions', 'targets'):
            out[f'{name}/cfg_{k}'] = np.array(cfg[k])
        out.update(r32)
        print(name, dict(zip(SUMMARY_KEYS, np.round(r32[f'{name}/summary'], 4).tolist())), flush=True)
        if name == 'default':
            none_valid = cat['gt'].copy()
            none_valid['valid'] = False
            try:
                with np.errstate(all='ignore'):
                    summarize(ref, none_valid, cat['matches'], cat['preds'], -1)
                raised = False
            except ZeroDivisionError:
                raised = True
            out['zero_valid_raises'] = np.array(raised)
            print('summary without a valid ground truth raises ZeroDivisionError:', raised)
    out.update(segmentation_cases(ref))
    path = HERE / 'reference_golden_det.npz'
    save_npz(path, out)
    print('wrote', path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()

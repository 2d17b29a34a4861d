"""Host half of the pose meter (cosypose_amd/pose_meters.py) without a device: grouping, filtering, matching, tables and summary
against the reference's own runs recorded in tests/golden/reference_golden_eval.npz (tests/golden/generate_golden_eval.py), fed
with the reference's float32 errors; the restated AUC / AP and the merge / fill rules on cases small enough to work out by hand.

Bounds: ids, flags and counts are compared exactly.  The summary's floats come from float64 host arithmetic on identical inputs on
both sides, so 1e-12 relative.  The generator asserts that no decision of these scenes (threshold, 0.1 d, AUC cut-off, choice
between two candidates, sphere test) is within 1e-3 of flipping and that all scores differ, so no case is left out.
"""
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import pose_meter_case as pc

SUMMARY_TOL = 1e-12


@pytest.fixture(scope='module')
def g():
    return pc.load()


def host_add(g, labels, infos, name, scene_id, a):
    """`add` with the device step replaced by the recorded errors -> (cand_infos, kept, matches, gt, preds)"""
    from cosypose_amd import pose_meters as pm
    kw = pc.meter_kwargs(g, labels, name)
    gt_infos, gt_poses, pred_infos, pred_poses = pc.frames(g, labels, scene_id)
    prep = pm.prepare_candidates(pred_infos, gt_infos, targets=kw['targets'], n_top=kw.get('n_top', -1), visib_gt_min=kw.get('visib_gt_min', -1),
                                 consider_all_predictions=kw.get('consider_all_predictions', False))
    assert np.array_equal(prep['keep_ids'], g[f'{name}/{a}/keep_ids']) and np.array_equal(prep['filtered_ids'], g[f'{name}/{a}/filtered_ids'])
    cand = prep['cand_infos']
    diameters = {l: infos[l]['diameter_m'] for l in labels}
    poses = pred_poses[prep['keep_ids']]
    if kw.get('spheres_overlap_check', True):
        filtered = poses[prep['filtered_ids']]
        cand = pm.spheres_overlap_filter(cand, filtered[cand['pred_id'].values, :3, 3], gt_poses[cand['gt_id'].values, :3, 3],
                                         [diameters[k] for k in cand['label']])
    matches, gt, preds, kept = pm.match_tables(cand, pc.recorded_errors(g, name, a), prep['pred_infos'], prep['gt_infos'], diameters,
                                               match_threshold=kw.get('match_threshold', 0.1), pred_poses=poses)
    return cand, kept, matches, gt, preds


@pytest.mark.parametrize('name', list(pc.CONFIGS))
def test_host_half_reproduces_the_reference_tables_and_summary(g, name):
    from cosypose_amd import pose_meters as pm
    labels, _, infos = pc.meshes(g)
    dfs = dict(gt=[], matches=[], preds=[])
    for a, scene_id in enumerate(g['scene_ids']):
        cand, kept, matches, gt, preds = host_add(g, labels, infos, name, scene_id, a)
        pc.check_candidates(g, name, a, cand, kept)
        got, want = pc.check_tables(g, name, a, cand, matches, gt, preds)
        assert np.array_equal(got, want)                    # the errors ARE the recorded ones: float32 values in float64 columns
        assert gt['norm'].dtype == np.float64 and gt['0.1d'].dtype == bool and gt['pred_inst_id'].dtype == np.float64
        dfs['gt'].append(gt); dfs['matches'].append(matches); dfs['preds'].append(preds)
    summary, out = pm.summarize(*(pd.concat(dfs[k], ignore_index=True) for k in ('gt', 'matches', 'preds')),
                                n_top=pc.CONFIGS[name].get('n_top', -1), report_AP=True, report_error_AUC=True, report_error_stats=True)
    print(name, {k: v for k, v in summary.items() if np.ndim(v) == 0})
    pc.check_summary(g, name, summary, lambda k: SUMMARY_TOL)
    want_auc = g[f'{name}/summary/AUC/labels']
    assert np.allclose(list(out['auc_objects'].values()), want_auc, rtol=SUMMARY_TOL, atol=0, equal_nan=True)
    want_ap = g[f'{name}/summary/AP/labels']
    got_ap = [np.unique(out['ap'][l]['AP']).item() if l in out['ap'] else np.nan for l in sorted(set(dfs['gt'][0]['label']) | set(dfs['gt'][1]['label']))]
    assert np.allclose(got_ap, want_ap, rtol=SUMMARY_TOL, atol=0, equal_nan=True)


def test_summary_keys_follow_the_report_flags(g):
    from cosypose_amd import pose_meters as pm
    labels, _, infos = pc.meshes(g)
    _, _, matches, gt, preds = host_add(g, labels, infos, 'addms', g['scene_ids'][0], 0)
    base = ['n_gt', 'n_gt_valid', 'n_pred', 'n_matched', 'matched_gt_ratio', 'pred_matched_ratio', '0.1d']
    assert list(pm.summarize(gt, matches, preds)[0]) == base
    assert list(pm.summarize(gt, matches, preds, report_error_stats=True, report_AP=True, report_error_AUC=True)[0]) == \
        base + ['norm', 'xyz', 'TCO_xyz', 'TCO_norm', 'AP', 'mAP', 'AUC/objects/mean', 'AUC']
    s = pm.summarize(gt, matches, preds)[0]
    assert s['pred_matched_ratio'] == len(preds) / len(matches)           # the reference's definition: predictions per match


# ---- restated metrics ------------------------------------------------------------------------------------------------------------------
def test_auc_posecnn_hand_cases():
    from cosypose_amd.pose_meters import compute_auc_posecnn as auc
    assert np.isnan(auc(np.array([np.inf, np.inf]))) and np.isnan(auc(np.array([]))) and np.isnan(auc(np.array([0.2, 0.5])))
    # the curve is integrated by the right-endpoint rule over [0, 0.1]: the stretch BEFORE an error already counts with that error's
    # accuracy (mrec / mpre of meters/utils.py:145-151), so a single matched error gives 1 whatever its value
    assert auc(np.array([0.02])) == pytest.approx(1.0, rel=1e-15)
    assert auc(np.array([0.02, np.inf])) == pytest.approx(0.5, rel=1e-15)
    # 0.02 and 0.06 of 4: 1/4 on [0, 0.02], 2/4 on [0.02, 0.06] and on [0.06, 0.1]
    assert auc(np.array([0.06, np.inf, 0.02, 0.3])) == pytest.approx((0.02 * 0.25 + 0.04 * 0.5 + 0.04 * 0.5) * 10, rel=1e-14)
    # equal errors: the first of them sets the stretch before, the last the stretch after; an error of exactly 0.1 stays in
    assert auc(np.array([0.05, 0.05])) == pytest.approx((0.05 * 0.5 + 0.05 * 1.0) * 10, rel=1e-14)
    assert auc(np.array([0.1])) == pytest.approx(1.0, rel=1e-15)
    assert auc(np.array([0.0])) == pytest.approx(1.0, rel=1e-15)
    e = np.array([0.03, 0.01])
    auc(e)
    assert list(e) == [0.03, 0.01]                                         # the input is not sorted in place


def test_auc_and_ap_against_recorded_reference_values(g):
    """per-label AUC (reference's compute_auc_posecnn) and AP (sklearn) of every recorded run, recomputed from the recorded columns"""
    from cosypose_amd.pose_meters import compute_auc_posecnn, average_precision
    labels, _, _ = pc.meshes(g)
    names = np.asarray(labels)
    n_checked = 0
    for name in pc.CONFIGS:
        gt_label = np.concatenate([names[g['gt_label'][g['gt_scene_id'] == s]] for s in g['scene_ids']])
        norm = np.concatenate([g[f'{name}/{a}/gt_norm'] for a in range(2)])
        valid = np.concatenate([g[f'{name}/{a}/gt_valid'] for a in range(2)])
        got = [compute_auc_posecnn(norm[valid & (gt_label == l)]) for l in sorted(set(gt_label[valid]))]
        assert np.allclose(got, g[f'{name}/summary/AUC/labels'], rtol=1e-12, atol=0, equal_nan=True)
        assert np.isclose(compute_auc_posecnn(norm[valid]), g[f'{name}/summary/AUC'][0], rtol=1e-12, atol=0)
        n_checked += len(got)
        # AP over all predictions: the recorded value is sklearn's AP x TP / n_gt_valid
        keep = [g[f'{name}/{a}/keep_ids'] for a in range(2)]
        score = np.concatenate([g['pred_score'][g['pred_scene_id'] == s][k] for s, k in zip(g['scene_ids'], keep)])
        tp = np.concatenate([g[f'{name}/{a}/preds_0.1d'] for a in range(2)])
        ap = average_precision(tp, score) * tp.sum() / g[f'{name}/summary/n_gt_valid'][0]
        assert np.isclose(ap, g[f'{name}/summary/AP'][0], rtol=1e-12, atol=0)
    assert n_checked >= 50


def test_average_precision_hand_cases():
    from cosypose_amd.pose_meters import average_precision as ap
    # scores all different: mean over the positives of the precision at each
    assert ap([1, 0, 1], [0.9, 0.8, 0.7]) == pytest.approx((1 + 2 / 3) / 2, rel=1e-15)
    assert ap([0, 1], [0.9, 0.1]) == pytest.approx(0.5, rel=1e-15)
    assert ap([1, 1], [0.3, 0.2]) == 1.0
    # equal scores share one threshold: {0.9: 1 of 1} then {0.5, 0.5: 2 of 3 so far}: 0.5 * 1 + 0.5 * 2/3
    assert ap([1, 1, 0], [0.9, 0.5, 0.5]) == pytest.approx(0.5 + 0.5 * 2 / 3, rel=1e-15)
    assert ap([1, 0, 1], [0.9, 0.5, 0.5]) == ap([1, 1, 0], [0.9, 0.5, 0.5])     # order inside a tie does not matter
    assert ap([1, 0, 1, 0], [0.5, 0.5, 0.5, 0.5]) == pytest.approx(0.5, rel=1e-15)
    assert np.isnan(ap([], []))


def tiny_tables(errors, scores=(0.9, 0.8, 0.7), gt_labels=('a', 'a', 'b'), pred_labels=('a', 'a', 'b'), threshold=0.1, **prep_kw):
    from cosypose_amd import pose_meters as pm
    gt = pd.DataFrame(dict(scene_id=1, view_id=0, label=list(gt_labels)))
    pred = pd.DataFrame(dict(scene_id=1, view_id=0, label=list(pred_labels), score=list(scores)))
    prep = pm.prepare_candidates(pred, gt, **prep_kw)
    cand = prep['cand_infos']
    n = len(cand)
    err = dict(norm_avg=np.asarray(errors, np.float32)[:n], xyz_avg=np.tile(np.asarray(errors, np.float32)[:n, None], (1, 3)),
               TCO_xyz=np.zeros((n, 3), np.float32), TCO_norm=np.zeros(n, np.float32))
    matches, gt_t, preds_t, kept = pm.match_tables(cand, err, prep['pred_infos'], prep['gt_infos'], dict(a=1.0, b=1.0), match_threshold=threshold)
    return cand, matches, gt_t, preds_t


def test_merge_and_fill_semantics_by_hand():
    """2 ground truths and 2 predictions of label a (4 candidates: p0g0 p0g1 p1g0 p1g1), one pair of label b"""
    cand, matches, gt, preds = tiny_tables([0.05, 0.02, 0.01, 0.5, 0.3])
    assert list(zip(cand['pred_id'], cand['gt_id'])) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]
    # p0 (score 0.9) goes first and takes g1 (0.02 < 0.05); p1 takes g0 (0.01); b's pair is over the threshold 0.1
    assert list(matches['cand_id']) == [1, 2] and list(matches['pred_inst_id']) == [0, 1] and list(matches['gt_inst_id']) == [1, 0]
    assert list(matches['score']) == [0.9, 0.8] and list(matches['0.1d']) == [True, True]
    assert np.allclose(gt['norm'].values[:2], [0.01, 0.02], rtol=1e-6) and gt['norm'].values[2] == np.inf
    assert list(gt['pred_inst_id'].values[:2]) == [1.0, 0.0] and np.isnan(gt['pred_inst_id'].values[2]) and np.isnan(gt['cand_id'].values[2])
    assert list(gt['0.1d']) == [True, True, False] and np.isnan(gt['score'].values[2]) and np.isnan(gt['obj_diameter'].values[2])
    assert np.all(np.isinf(gt['xyz'].values[2])) and gt['xyz'].values[2].shape == (3,) and np.all(np.isnan(gt['TXO_pred'].values[2]))
    assert np.all(np.isinf(gt['TCO_xyz'].values[2])) and gt['TCO_norm'].values[2] == np.inf
    assert list(preds['0.1d']) == [True, True, False]
    assert 'visib_fract' not in gt


def test_greedy_matching_by_hand():
    # the better-scored prediction takes the ground truth both want; the other falls back to its second choice or stays unmatched
    _, matches, gt, _ = tiny_tables([0.01, 0.05, 0.02, 0.5, 0.3], threshold=0.1)
    assert list(matches['cand_id']) == [0]                       # p0 -> g0; p1's only candidate within the threshold is g0: taken
    assert gt['norm'].values[1] == np.inf
    _, matches, _, _ = tiny_tables([0.01, 0.05, 0.02, 0.5, 0.3], threshold=0.6)
    assert list(matches['cand_id']) == [0, 3, 4]                 # now p1 falls back to g1 (0.5), and b matches
    _, matches, _, _ = tiny_tables([0.01, 0.05, 0.02, 0.5, 0.3], scores=(0.1, 0.8, 0.7), threshold=0.6, consider_all_predictions=True)
    assert list(matches['cand_id']) == [2, 1, 4]                 # (rows kept in the given order) p1 first: g0 (0.02); p0 falls back to g1 (0.05)
    _, matches, _, _ = tiny_tables([0.04, 0.04, 0.3, 0.3, 0.3])
    assert list(matches['cand_id']) == [0]                       # equal errors: the first candidate wins
    _, matches, _, _ = tiny_tables([np.nan, 0.04, 0.3, 0.3, 0.3])
    assert list(matches['cand_id']) == [1]                       # a NaN error never matches
    _, matches, gt, preds = tiny_tables([0.5, 0.5, 0.5, 0.5, 0.5])
    assert len(matches) == 0 and np.all(np.isinf(gt['norm'])) and not preds['0.1d'].any()


def test_filters_by_hand():
    from cosypose_amd import pose_meters as pm
    gt = pd.DataFrame(dict(scene_id=[1, 1, 1, 2], view_id=[0, 0, 0, 0], label=['a', 'a', 'b', 'a'], visib_fract=[0.2, 0.9, 0.5, 0.7]))
    pred = pd.DataFrame(dict(scene_id=[2, 1, 1, 1, 9], view_id=[0, 0, 0, 0, 0], label=['a', 'a', 'a', 'c', 'a'], score=[0.5, 0.2, 0.6, 0.9, 0.99]))
    prep = pm.prepare_candidates(pred, gt)
    assert list(prep['keep_ids']) == [1, 2, 3, 0]                # the ground truth's (scene, view) order; scene 9 has no ground truth
    assert list(prep['pred_infos']['pred_inst_id']) == [0, 1, 0, 0]
    assert list(prep['filtered_ids']) == [1, 0, 2, 3]            # groups in key order, best score first
    assert list(prep['gt_infos']['gt_inst_id']) == [0, 1, 0, 0] and prep['gt_infos']['valid'].all()
    assert len(prep['cand_infos']) == 5
    assert list(pm.prepare_candidates(pred, gt, n_top=1)['filtered_ids']) == [1, 2, 3]
    assert list(pm.prepare_candidates(pred, gt, consider_all_predictions=True, n_top=1)['filtered_ids']) == [0, 1, 2, 3]
    targets = pd.DataFrame(dict(scene_id=[1, 1], view_id=[0, 0], label=['a', 'b'], inst_count=[1, 1]))
    prep = pm.prepare_candidates(pred, gt, targets=targets)
    assert list(prep['filtered_ids']) == [1]                     # one a of scene 1; c and scene 2 are no targets
    assert list(prep['gt_infos']['valid']) == [False, True, True, False]      # the most visible a, and b
    prep = pm.prepare_candidates(pred, gt, targets=targets, visib_gt_min=0.4)
    assert list(prep['gt_infos']['valid']) == [False, True, True, True]       # visible enough and of a target LABEL (scene 2's a too)
    # sphere test: strict <, per pair
    cand = pd.DataFrame(dict(pred_id=[0, 1, 2], gt_id=[0, 0, 0], cand_id=[0, 1, 2]))
    out = pm.spheres_overlap_filter(cand, np.array([[0.1, 0, 0], [0.2, 0, 0], [0, 0.3, 0.4]]), np.zeros((3, 3)), [0.2, 0.2, 0.6])
    assert list(out['pred_id']) == [0, 2] and list(out['cand_id']) == [0, 1]


def test_no_matches_and_no_predictions():
    from cosypose_amd import pose_meters as pm
    _, matches, gt, preds = tiny_tables([0.5] * 5)
    s, _ = pm.summarize(gt, matches, preds, report_AP=True, report_error_AUC=True, report_error_stats=True)
    assert s['AP'] == 0. and s['mAP'] == 0. and s['n_matched'] == 0 and s['pred_matched_ratio'] == 3.0 and s['0.1d'] == 0.
    assert np.isnan(s['AUC']) and np.isnan(s['AUC/objects/mean']) and np.isnan(s['norm']) and np.all(np.isnan(s['xyz']))
    _, matches, gt, preds = tiny_tables([], scores=(), pred_labels=())
    assert len(preds) == 0 and len(matches) == 0 and len(gt) == 3
    s, _ = pm.summarize(gt, matches, preds, report_AP=True, report_error_AUC=True)
    assert s['n_pred'] == 0 and s['n_gt_valid'] == 3 and s['AP'] == 0. and s['mAP'] == 0. and s['matched_gt_ratio'] == 0.


def test_n_top_changes_the_ground_truth_count():
    from cosypose_amd import pose_meters as pm
    _, matches, gt, preds = tiny_tables([0.05, 0.02, 0.01, 0.5, 0.3])
    assert pm.summarize(gt, matches, preds)[0]['n_gt_valid'] == 3
    s = pm.summarize(gt, matches, preds, n_top=1)[0]
    assert s['n_gt_valid'] == 2 and s['n_gt'] == 3 and s['matched_gt_ratio'] == 1.0     # one per (scene, view, label) group


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES
    build()
    for name in ('cosy_pose_errors', 'cosy_pose_errors_workspace_bytes'):
        assert name in _lib.EXPORTS           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_eval.hip' in SOURCES
    import cosypose_amd
    from cosypose_amd import pose_meters, distances
    assert cosypose_amd.PoseErrorMeter is pose_meters.PoseErrorMeter and callable(distances.pose_errors)
    for method in ('add', 'summary', 'reset', 'is_data_valid'):
        assert callable(getattr(pose_meters.PoseErrorMeter, method))
    # argument checks that need no device: refused before any launch
    l = _lib.lib()
    assert l.cosy_pose_errors_workspace_bytes(0, 100) == 0 and l.cosy_pose_errors_workspace_bytes(4, 1025) >= 4 * 2 * 32 + 20
    none6 = [None] * 6
    assert l.cosy_pose_errors(*none6, 0, 1, 1, None, None, 0, None) == 0                # B = 0 with null pointers
    assert l.cosy_pose_errors(*none6, -1, 1, 1, None, None, 0, None) == -1 and b'B=-1' in l.cosy_last_error()
    assert l.cosy_pose_errors(*none6, 1, 0, 1, None, None, 0, None) == -1 and b'n_obj=0' in l.cosy_last_error()
    assert l.cosy_pose_errors(*none6, 1, 1, 0, None, None, 0, None) == -1 and b'n_max=0' in l.cosy_last_error()
    assert l.cosy_pose_errors(*none6, 1, 1, 1, None, None, 0, None) == -1 and b'null TXO_pred' in l.cosy_last_error()


def test_product_imports_no_xarray_sklearn_scipy_or_oracle():
    code = ('import sys; import cosypose_amd.pose_meters, cosypose_amd.distances; '
            'bad = [m for m in sys.modules if m.split(".")[0] in ("xarray", "sklearn", "scipy", "cosy_oracle")]; print(bad); sys.exit(bool(bad))')
    from conftest import REPO
    r = subprocess.run([sys.executable, '-c', code], cwd=str(REPO), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for f in ('pose_meters.py', 'distances.py'):
        text = (REPO / 'cosypose_amd' / f).read_text()
        assert not re.search(r'^\s*(import|from)\s+(xarray|sklearn|scipy|cosy_oracle)', text, flags=re.M)

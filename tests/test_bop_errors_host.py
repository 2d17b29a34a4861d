"""CPU tests of the BOP errors and scores: the numpy twins (tests/bop_ref.py) against hand values, the host halves of
cosypose_amd/bop_errors.py and bop_meters.py (window planning, matching, recall, summary) on tables alone, and the C ABI's host-side
argument checks.  No GPU."""
import pathlib

import numpy as np
import pandas as pd
import pytest
import torch

import bop_ref as br

REPO = pathlib.Path(__file__).resolve().parent.parent
DELTA = 0.015


# ---- the twins against hand values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', br.hand_cases(), ids=lambda c: c[0])
def test_vsd_hand_values(case):
    name, D_est, D_gt, D_test, taus, want = case
    c64 = br.vsd_counts64(D_est, D_gt, D_test, br.HAND_K, taus, DELTA)
    e = br.vsd_from_counts(c64)
    print(name, 'counts', c64, 'e', e)
    assert e.shape == (1,) and abs(e[0] - want) < 1e-15
    # the float32 twin decides every pixel as the float64 twin does, and no pixel of a hand case is near a threshold
    assert np.array_equal(br.vsd_counts32(D_est, D_gt, D_test, br.HAND_K, taus, DELTA), c64)
    lo, hi, undecided, union = br.vsd_intervals64(D_est, D_gt, D_test, br.HAND_K, taus, DELTA)
    assert undecided == 0 and np.array_equal(lo, c64) and np.array_equal(hi, c64) and union == c64[0]


def test_vsd_counts_of_several_taus_and_an_undecided_pixel():
    gt, est = br.square(1.0, 16, 32), br.square(1.03, 16, 32)
    taus = [0.01, 0.02, 0.04, 0.5]
    c = br.vsd_counts64(est, gt, gt, br.HAND_K, taus, DELTA)
    assert c[0] == c[1] == 256 and list(c[2:]) == [256, 256, 0, 0]
    assert np.allclose(br.vsd_from_counts(c), [1, 1, 0, 0])
    # a tau exactly at one pixel's |dist_gt - dist_est| makes that pixel (and its mirror images, if any) undecided
    diff = np.abs(br.dist64(gt, br.HAND_K) - br.dist64(est, br.HAND_K))
    tau = np.float32(diff[20, 20])
    lo, hi, undecided, union = br.vsd_intervals64(est, gt, gt, br.HAND_K, [tau], DELTA)
    assert undecided >= 1 and np.all(hi - lo == undecided) and union == 256


def test_distance_image_float32_against_float64_within_six_roundings():
    rs = np.random.RandomState(0)
    depth = rs.uniform(0.3, 3.0, (96, 128)).astype(np.float32)
    K = br.make_K(1, 96, 128)[0]
    d32, d64 = br.dist32(depth, K), br.dist64(depth, K)
    worst = np.max(np.abs(d32 - d64) / d64) / br.U
    print('worst |dist32 - dist64| / (u dist):', worst)
    assert d32.dtype == np.float32 and worst <= 6


def test_mssd_of_a_translation_and_of_a_listed_symmetry():
    rs = np.random.RandomState(1)
    verts = (rs.uniform(-1, 1, (200, 3)) * [0.05, 0.08, 0.03]).astype(np.float32)
    K = br.make_K(1, 480, 640)[0]
    Tg = br.rand_pose(rs, 1)[0]
    t = np.array([0.01, -0.02, 0.015])
    Tp = Tg.astype(np.float64).copy(); Tp[:3, 3] += t
    mssd, _ = br.mssd_mspd64(Tp.astype(np.float32), Tg, K, verts, np.eye(4)[None])
    assert abs(mssd - np.linalg.norm(Tp.astype(np.float32)[:3, 3].astype(np.float64) - Tg[:3, 3])) < 1e-12
    # an estimate turned by a listed symmetry: 0 with it, > 0 without (the symmetry is exact in float32: a half turn)
    half = br.rot_z(np.pi).round()
    Tp = (Tg.astype(np.float64) @ half).astype(np.float32)
    with_sym, _ = br.mssd_mspd64(Tp, Tg, K, verts, np.stack([np.eye(4), half]))
    without, _ = br.mssd_mspd64(Tp, Tg, K, verts, np.eye(4)[None])
    assert with_sym == 0.0 and without > 0.05


def test_mspd_of_a_sideways_shift_of_a_plane():
    rs = np.random.RandomState(2)
    verts = np.concatenate([rs.uniform(-0.1, 0.1, (50, 2)), np.zeros((50, 1))], 1).astype(np.float32)
    K = br.make_K(1, 480, 640)[0]
    Tg = np.eye(4, dtype=np.float32); Tg[2, 3] = 0.75
    Tp = Tg.copy(); Tp[0, 3] = 0.03125
    _, mspd = br.mssd_mspd64(Tp, Tg, K, verts, np.eye(4)[None])
    assert abs(mspd - float(K[0, 0]) * 0.03125 / 0.75) < 1e-9


# ---- matching and recall on hand tables ------------------------------------------------------------------------------------------------------
def both(cand, n_valid, err, theta):
    """the package's match_counts (one setting per column) and the twin's loops must agree -> {group: matched} per column"""
    from cosypose_amd.bop_meters import match_counts
    err, theta = np.asarray(err, np.float64).reshape(len(cand), -1), np.asarray(theta, np.float64).reshape(len(cand), -1)
    got = match_counts([c[0] for c in cand], [c[1] for c in cand], [c[2] for c in cand], [c[3] for c in cand], n_valid, err, theta)
    cols = []
    for k in range(err.shape[1]):
        want = br.match_recall(cand, n_valid, err[:, k], theta[:, k])
        assert {g: int(v[k]) for g, v in got.items()} == want, (k, got, want)
        cols.append(want)
    return cols


def test_matching_caps_the_predictions_at_the_number_of_valid_ground_truths():
    # one group, one valid ground truth (row 0), two predictions: the better-scored one misses, the other would hit but is never used
    cand = [(0, 0, 0, 0.9), (0, 1, 0, 0.8)]
    assert both(cand, {0: 1}, [0.5, 0.01], [0.1, 0.1]) == [{0: 0}]
    assert both(cand, {0: 2}, [0.5, 0.01], [0.1, 0.1]) == [{0: 1}]            # with n = 2 the second prediction is used


def test_matching_score_ties_go_to_the_lower_prediction_row():
    # equal scores, n = 1: prediction row 3 is used, row 7 is not -- whichever comes first in the table
    for cand in ([(0, 7, 0, 0.5), (0, 3, 0, 0.5)], [(0, 3, 0, 0.5), (0, 7, 0, 0.5)]):
        err = [0.01 if c[1] == 7 else 0.5 for c in cand]
        assert both(cand, {0: 1}, err, [0.1, 0.1]) == [{0: 0}]
        err = [0.01 if c[1] == 3 else 0.5 for c in cand]
        assert both(cand, {0: 1}, err, [0.1, 0.1]) == [{0: 1}]


def test_two_predictions_compete_for_one_ground_truth():
    # ground truths 0 and 1; prediction 0 (best score) is within the threshold of both and nearer to 0; prediction 1 only of 0
    cand = [(0, 0, 0, 0.9), (0, 0, 1, 0.9), (0, 1, 0, 0.8), (0, 1, 1, 0.8)]
    assert both(cand, {0: 2}, [0.01, 0.02, 0.03, 0.5], [0.1] * 4) == [{0: 1}]
    # the other way round prediction 0 takes ground truth 1 and leaves 0 to prediction 1
    assert both(cand, {0: 2}, [0.02, 0.01, 0.03, 0.5], [0.1] * 4) == [{0: 2}]
    # equal errors: the lower ground-truth row is taken, prediction 1 then finds ground truth 1 out of reach
    assert both(cand, {0: 2}, [0.02, 0.02, 0.03, 0.5], [0.1] * 4) == [{0: 1}]
    # strict <, NaN below nothing, and several settings at once
    err = np.array([[0.1, 0.1, np.nan], [0.5, 0.05, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.01]])
    theta = np.array([[0.1, 0.2, 0.2]] * 4)
    assert both(cand, {0: 2}, err, theta) == [{0: 0}, {0: 1}, {0: 1}]


def frames_of_hand_scene():
    """two groups with ground truth (label a: two instances, one not valid; label b: one), predictions of a, b and of label c,
    which has no ground truth"""
    gt = pd.DataFrame(dict(scene_id=[1, 1, 1], view_id=[0, 0, 0], label=['a', 'a', 'b'], visib_fract=[0.9, 0.05, 0.5]))
    pred = pd.DataFrame(dict(scene_id=[1, 1, 1, 1], view_id=[0, 0, 0, 0], label=['a', 'a', 'b', 'c'], score=[0.9, 0.8, 0.7, 0.6]))
    return gt, pred


def test_group_table_and_summary_on_hand_tables():
    from cosypose_amd.pose_meters import prepare_candidates
    from cosypose_amd.bop_meters import group_table, summarize, BopScoreMeter
    gt, pred = frames_of_hand_scene()
    prep = prepare_candidates(pred, gt, visib_gt_min=0.1)
    cand = prep['cand_infos']
    assert list(cand['label']) == ['a', 'a', 'b'] and list(cand['gt_id']) == [0, 0, 2]          # the invalid instance and label c give no pairs
    n = len(cand)
    # label a: its best-scored prediction is far off, the second one (never used: n = 1) would be right; label b: right under every setting
    errors = dict(vsd=np.array([[0.9] * 10, [0.0] * 10, [0.0] * 10]), mssd=np.array([1.0, 0.0, 0.0]), mspd=np.array([500.0, 0.0, 0.0]))
    groups = group_table(cand, prep['gt_infos'], errors, np.full(n, 0.2), 640)
    assert list(groups['label']) == ['a', 'b'] and list(groups['n_valid']) == [1, 1]
    assert groups['matched_vsd'][0].shape == (100,) and groups['matched_mssd'][0].shape == (10,) and groups['matched_mspd'][0].shape == (10,)
    assert not groups['matched_vsd'][0].any() and groups['matched_vsd'][1].all() and groups['matched_mssd'][1].all()
    summary, dfs = summarize(groups)
    assert summary['n_gt_valid'] == 2 and summary['AR_VSD'] == 0.5 and summary['AR_MSSD'] == 0.5 and summary['AR_MSPD'] == 0.5 and summary['AR'] == 0.5
    assert summary['AR/objects/a'] == 0.0 and summary['AR/objects/b'] == 1.0 and 'AR/objects/c' not in summary
    assert list(dfs['labels']['label']) == ['a', 'b']
    # the meter's summary: the same keys plus the counts of what was added
    meter = BopScoreMeter(models=None)
    assert meter.visib_gt_min == 0.1
    meter.datas['groups'].append(groups); meter.datas['n_gt'] += 3; meter.datas['n_pred'] += 4
    summary, dfs = meter.summary()
    for k in ('AR', 'AR_VSD', 'AR_MSSD', 'AR_MSPD', 'n_gt', 'n_gt_valid', 'n_pred', 'AR_VSD/objects/a', 'AR_MSSD/objects/b', 'AR_MSPD/objects/b'):
        assert k in summary, k
    assert summary['n_gt'] == 3 and summary['n_pred'] == 4 and set(dfs) == {'groups', 'labels'}
    # the twin's scores on the same tables
    c = [(0 if l == 'a' else 1, p, g, s) for l, p, g, s in zip(cand['label'], cand['pred_id'], cand['gt_id'], cand['score'])]
    want = br.bop_scores(c, None, {0: 1, 1: 1}, {0: 'a', 1: 'b'}, errors['vsd'], errors['mssd'], errors['mspd'], np.full(n, 0.2), 640)
    assert want['all']['AR'] == summary['AR'] and want['a']['AR'] == summary['AR/objects/a'] and want['b']['AR_VSD'] == summary['AR_VSD/objects/b']


def test_an_add_without_a_tentative_pair_counts_its_ground_truth_with_zero_matches():
    """no prediction's label has valid ground truth: the groups are still recorded, recall over them is 0"""
    from cosypose_amd.pose_meters import prepare_candidates
    from cosypose_amd.bop_meters import group_table, summarize
    gt = pd.DataFrame(dict(scene_id=[1, 1], view_id=[0, 0], label=['a', 'b'], visib_fract=[0.9, 0.9]))
    pred = pd.DataFrame(dict(scene_id=[1], view_id=[0], label=['c'], score=[0.5]))
    prep = prepare_candidates(pred, gt, visib_gt_min=0.1)
    assert len(prep['cand_infos']) == 0
    empty = dict(vsd=np.zeros((0, 10)), mssd=np.zeros(0, np.float32), mspd=np.zeros(0, np.float32))       # what bop_errors returns for B = 0
    groups = group_table(prep['cand_infos'], prep['gt_infos'], empty, np.zeros(0), 640)
    assert list(groups['label']) == ['a', 'b'] and list(groups['n_valid']) == [1, 1]
    assert groups['matched_vsd'][0].shape == (100,) and not any(groups[c][g].any() for c in ('matched_vsd', 'matched_mssd', 'matched_mspd') for g in (0, 1))
    summary, _ = summarize(groups)
    assert summary['n_gt_valid'] == 2 and summary['AR'] == 0.0 and summary['AR_VSD'] == 0.0 and summary['AR_MSSD/objects/b'] == 0.0
    # together with an add that matches everything: the empty add's ground truth stays in the denominator
    gt2, pred2 = frames_of_hand_scene()
    prep2 = prepare_candidates(pred2, gt2, visib_gt_min=0.1)
    errors = dict(vsd=np.zeros((3, 10)), mssd=np.zeros(3), mspd=np.zeros(3))
    both_adds = pd.concat([groups, group_table(prep2['cand_infos'], prep2['gt_infos'], errors, np.full(3, 0.2), 640)], ignore_index=True)
    assert summarize(both_adds)[0]['AR'] == 0.5


def test_thresholds_scale_with_diameter_and_image_width():
    from cosypose_amd.bop_meters import settings_tables
    from cosypose_amd import bop_errors as be
    assert be.VSD_DELTA == 0.015 and be.VSD_TAUS == be.VSD_THRESHOLDS == be.MSSD_THRESHOLDS == (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)
    assert be.MSPD_THRESHOLDS == (5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 50.0)
    t = settings_tables(dict(vsd=np.arange(20.).reshape(2, 10), mssd=[1., 2.], mspd=[3., 4.]), [0.1, 0.2], 1280)
    err, theta = t['vsd']
    assert err.shape == theta.shape == (2, 100) and list(err[0, :11]) == [0.] * 10 + [1.] and list(theta[1, 9:12]) == [0.5, 0.05, 0.1]
    assert np.allclose(t['mssd'][1], np.outer([0.1, 0.2], be.MSSD_THRESHOLDS)) and np.allclose(t['mspd'][1][0], 2 * np.asarray(be.MSPD_THRESHOLDS))


# ---- the host half of the device call ----------------------------------------------------------------------------------------------------
def test_vsd_from_counts_and_absolute_taus():
    from cosypose_amd.bop_errors import vsd_from_counts, absolute_taus
    counts = np.array([[10, 4, 0, 2, 4], [0, 0, 0, 0, 0], [7, 7, 7, 3, 0]])
    want = br.vsd_from_counts(counts)
    assert np.array_equal(vsd_from_counts(counts), want) and want[1].tolist() == [1, 1, 1] and want[0].tolist() == [0.6, 0.8, 1.0]
    got = vsd_from_counts(torch.from_numpy(counts).to(torch.int32))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    taus = absolute_taus((0.05, 0.5), [1, 0, 1], [0.2, 0.3])
    assert taus.dtype == np.float32 and np.array_equal(taus, np.array([[0.05 * 0.3, 0.5 * 0.3], [0.05 * 0.2, 0.5 * 0.2], [0.05 * 0.3, 0.5 * 0.3]]).astype(np.float32))
    assert np.array_equal(absolute_taus(np.full((3, 2), 0.25), [1, 0, 1], [0.2, 0.3]), np.full((3, 2), 0.25, np.float32))
    with pytest.raises(AssertionError):
        absolute_taus(np.linspace(0.01, 0.5, 17), [0], [0.2])


def test_plan_windows_chunks_under_a_cap():
    from cosypose_amd.bop_errors import plan_windows
    boxes = np.array([[0, 0, 9, 9], [5, 5, 4, 9], [2, 3, 2, 3], [0, 0, 19, 4], [1, 1, 10, 10]])          # 100, empty, 1, 100, 100 pixels
    est, gt = np.array([0, 1, 3, 4]), np.array([2, 2, 2, 0])
    one = plan_windows(boxes, est, gt)
    assert len(one) == 1 and one[0]['n_pixels'] == 301 and list(one[0]['win_offset']) == [0, -1, 100, 101, 201] and (one[0]['lo'], one[0]['hi']) == (0, 4)
    assert len(plan_windows(boxes, est, gt, 301)) == 1
    parts = plan_windows(boxes, est, gt, 201)
    assert [(c['lo'], c['hi'], c['n_pixels']) for c in parts] == [(0, 3, 201), (3, 4, 200)]
    assert list(parts[1]['win_offset']) == [0, -1, -1, -1, 100]
    for c in parts:          # every window lies inside its chunk's store and no two overlap
        size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
        used = np.flatnonzero(c['win_offset'] >= 0)
        spans = sorted((c['win_offset'][n], c['win_offset'][n] + size[n]) for n in used)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == c['n_pixels']
    with pytest.raises(ValueError, match='pair 3 alone needs 200'):
        plan_windows(boxes, est, gt, 150)
    assert plan_windows(boxes, est[:0], gt[:0]) == []


def test_bop_models_tables():
    from cosypose_amd import BopModels, BatchedMeshes, synthetic as syn
    verts, faces, colors = syn.make_render_meshes(3, 2, 6, 8)
    verts[1], colors[1] = verts[1][:30], colors[1][:30]
    faces[1] = faces[1][(faces[1] < 30).all(1)]
    half = br.rot_z(np.pi).round()
    m = BopModels(['a', 'b'], verts, faces, symmetries=[None, np.stack([np.eye(4), half])], colors_list=colors)
    assert m.n_verts.tolist() == [42, 30] and m.n_sym.tolist() == [1, 2] and m.sym_table.shape == (2, 2, 4, 4)
    assert torch.equal(m.sym_table[0, 1], torch.eye(4)) and np.array_equal(m.sym_table[1, 1].numpy(), half.astype(np.float32))
    assert m.meshes.verts.shape == (2, 42, 3) and m.diameters.shape == (2,) and m.label_to_id == {'a': 0, 'b': 1}
    assert abs(m.diameters[0] - np.linalg.norm(verts[0].astype(np.float64).max(0) - verts[0].astype(np.float64).min(0))) < 1e-12
    with pytest.raises(AssertionError, match='identity'):
        BopModels(['a'], verts[:1], faces[:1], symmetries=[half[None]])
    infos = {'a': dict(n_sym=1, diameter_m=0.25), 'b': dict(n_sym=2, diameter_m=0.5)}
    db = BatchedMeshes(infos, ['a', 'b'], torch.zeros(2, 5, 3), torch.from_numpy(np.stack([np.stack([np.eye(4), half])] * 2)).float())
    m = BopModels.from_mesh_db(db, verts, faces)
    assert m.n_sym.tolist() == [1, 2] and m.diameters.tolist() == [0.25, 0.5]


def test_package_exports():
    import cosypose_amd
    from cosypose_amd import bop_errors, BopModels, BopScoreMeter
    assert callable(bop_errors) and callable(cosypose_amd.bop_errors) and BopModels is bop_errors.BopModels
    assert BopScoreMeter.__module__ == 'cosypose_amd.bop_meters'


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
BOP_SYMBOLS = ('cosy_bop_mssd_mspd_workspace_bytes', 'cosy_bop_mssd_mspd', 'cosy_bop_instance_boxes', 'cosy_bop_windows_workspace_bytes',
               'cosy_bop_render_windows', 'cosy_bop_vsd_workspace_bytes', 'cosy_bop_vsd_counts')


def test_c_abi_declares_exports_and_builds_the_bop_entry_points():
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES, FILE_FLAGS
    build()
    for name in BOP_SYMBOLS:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_bop.hip' in SOURCES and '-ffp-contract=off' in FILE_FLAGS['kernels_bop.hip']


def test_argument_checks_run_on_the_host_before_any_launch():
    """COSY_EINVAL (-1) with the argument named, and B = 0 / N = 0 return COSY_OK with null pointers: neither touches a device"""
    from cosypose_amd._lib import lib
    l = lib()
    P = 64          # a non-null, 16-byte aligned stand-in: every call below is refused (or returns) before a pointer is used
    assert l.cosy_bop_mssd_mspd_workspace_bytes(0, 4) == 0 and l.cosy_bop_mssd_mspd_workspace_bytes(3, 5) >= 3 * 5 * 8 + 16
    assert l.cosy_bop_windows_workspace_bytes(0) == 0 and l.cosy_bop_windows_workspace_bytes(5) == 32 and l.cosy_bop_vsd_workspace_bytes(0) == 0
    assert l.cosy_bop_vsd_workspace_bytes(7) % 16 == 0 and l.cosy_bop_vsd_workspace_bytes(7) >= 8 + 8 * 4

    def mssd(**kw):
        a = dict(p=P, g=P, o=P, v=P, K=P, x=P, nv=P, s=P, ns=P, B=2, n_obj=1, n_views=1, V=10, S=2, e3=P, e2=P, ws=P, wb=1 << 20, st=None)
        a.update(kw)
        return l.cosy_bop_mssd_mspd(*a.values())
    for bad, word in ((dict(B=-1), b'B=-1'), (dict(n_obj=0), b'n_obj=0'), (dict(n_views=0), b'n_views=0'), (dict(V=0), b'V=0'), (dict(S=0), b'S=0'),
                      (dict(p=None), b'null TCO_pred'), (dict(g=None), b'null TCO_gt'), (dict(o=None), b'null obj_id'), (dict(v=None), b'null view_id'),
                      (dict(K=None), b'null K'), (dict(x=None), b'null verts'), (dict(nv=None), b'null n_verts'), (dict(s=None), b'null sym_table'),
                      (dict(ns=None), b'null n_sym'), (dict(e3=None), b'null mssd'), (dict(e2=None), b'null mspd'), (dict(ws=None), b'null workspace'),
                      (dict(wb=8), b'workspace_bytes=8'), (dict(ws=P + 4), b'16-byte'), (dict(B=1 << 30, V=5000), b'2^31')):
        assert mssd(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    assert mssd(B=0, p=None, g=None, o=None, v=None, K=None, x=None, nv=None, s=None, ns=None, e3=None, e2=None, ws=None, wb=0) == 0

    def boxes(**kw):
        a = dict(T=P, o=P, v=P, K=P, x=P, nv=P, N=2, n_obj=1, n_views=1, V=10, H=48, W=64, b=P, st=None)
        a.update(kw)
        return l.cosy_bop_instance_boxes(*a.values())
    for bad, word in ((dict(N=-1), b'N=-1'), (dict(H=0), b'H=0'), (dict(W=0), b'W=0'), (dict(V=0), b'V=0'), (dict(T=None), b'null TCO'),
                      (dict(b=None), b'null boxes'), (dict(nv=None), b'null n_verts')):
        assert boxes(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    assert boxes(N=0, T=None, o=None, v=None, K=None, x=None, nv=None, b=None) == 0

    def windows(**kw):
        a = dict(T=P, o=P, v=P, K=P, x=P, f=P, nf=P, b=P, off=P, N=2, n_obj=1, n_views=1, V=10, F=10, H=48, W=64, n_px=100, ws=P, wb=400, st=None)
        a.update(kw)
        return l.cosy_bop_render_windows(*a.values())
    for bad, word in ((dict(N=-1), b'N=-1'), (dict(F=0), b'F=0'), (dict(n_px=-1), b'n_pixels=-1'), (dict(f=None), b'null faces'),
                      (dict(nf=None), b'null n_faces'), (dict(off=None), b'null win_offset'), (dict(ws=None), b'null workspace'),
                      (dict(wb=399), b'workspace_bytes=399'), (dict(ws=P + 8), b'16-byte')):
        assert windows(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    assert windows(N=0, T=None, o=None, v=None, K=None, x=None, f=None, nf=None, b=None, off=None, ws=None, wb=0) == 0
    assert windows(n_px=0, ws=None, wb=0) == 0

    def vsd(**kw):
        a = dict(e=P, g=P, iv=P, b=P, off=P, w=P, n_px=100, d=P, K=P, t=P, delta=0.015, B=2, N=3, n_views=1, n_tau=10, H=48, W=64, c=P, ws=P, wb=64,
                 st=None)
        a.update(kw)
        return l.cosy_bop_vsd_counts(*a.values())
    for bad, word in ((dict(B=-1), b'B=-1'), (dict(n_tau=0), b'n_tau=0'), (dict(n_tau=17), b'n_tau=17'), (dict(e=None), b'null est_inst'),
                      (dict(g=None), b'null gt_inst'), (dict(d=None), b'null depth_test'), (dict(t=None), b'null taus'), (dict(c=None), b'null counts'),
                      (dict(iv=None), b'null inst_view'), (dict(w=None), b'null windows'), (dict(ws=None), b'null workspace'),
                      (dict(wb=8), b'workspace_bytes=8'), (dict(ws=P + 4), b'16-byte')):
        assert vsd(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    assert vsd(B=0, e=None, g=None, iv=None, b=None, off=None, w=None, d=None, K=None, t=None, c=None, ws=None, wb=0) == 0

"""Multi-view candidate matching on the GPU (cosypose_amd/multiview_matching.py, csrc/kernels_ransac.hip) against the reference's own
float32 runs in tests/golden/reference_golden_ransac.npz (tests/golden/generate_golden_ransac.py).

The reference does not determine single hypotheses to rounding (when the two matches of a seed share a candidate every symmetry of
the label gives the same minimum, so the last bit picks the symmetry: 12-32 % of all hypotheses), so the comparison is STAGED: each
stage gets the reference's inputs for that stage, and the bounds are the ones the project applies to its float32 distances (1e-5)
with a 1e-4 band around decisions.  Every test prints its figures before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import ransac_case as rc

pytestmark = pytest.mark.gpu

DIST_TOL = 1e-5          # float32 distances (metres), the bound of cosy_symmetric_distance's tests
NEAR = 1e-4              # band around a decision (threshold, tie) inside which the reference itself is not determined
THRESHOLD = 0.02
N_MIN_INLIERS = 3


@pytest.fixture(scope='module')
def g():
    return rc.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene_tables(g, prefix):
    scene = rc.scene_of(g, prefix)
    return scene['cand_poses'].astype(np.float32), scene['sym'].astype(np.float32), scene['cand_label_id']


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_stage1_hypotheses(g, prefix):
    """Reference seeds in.  For EVERY seed TC1C2 == TC1Oa S_k inv(TC2Ob) for the returned k (1e-5); where the reference's runner-up gap
    is >= 1e-4, k and TC1C2 are the reference's; elsewhere k is a symmetry whose distance in the reference's own row is within 1e-4
    of that row's minimum.  Own distances per symmetry against the reference's: 1e-5.
    Measured on an MI355X: see DESIGN.md section 11."""
    from cosypose_amd.multiview_matching import estimate_camera_poses, estimate_camera_poses_batch
    cand, _, mesh_db = rc.collections(g, prefix, 'cuda')
    seeds = rc.seeds_of(g, prefix)
    out = estimate_camera_poses(cand, seeds, mesh_db)
    TC1C2, k, gap, rows = out['TC1C2'].cpu().numpy(), out['best_sym'].cpu().numpy(), out['gap'].cpu().numpy(), out['sym_dists'].cpu().numpy()
    poses, sym, label = scene_tables(g, prefix)
    a, b = seeds['match1_cand1'], seeds['match1_cand2']
    assert k.min() >= 0 and np.all(k < rc.scene_of(g, prefix)['n_sym'][label[a]])
    inv_b = np.linalg.inv(poses[b].astype(np.float64))
    built = poses[a].astype(np.float64) @ sym[label[a], k].astype(np.float64) @ inv_b
    ref_rows, ref_k, ref_gap = g[prefix + 'sym_dists'], g[prefix + 'sym'], g[prefix + 'gap']
    clear = ref_gap >= NEAR
    finite = np.isfinite(ref_rows)
    figs = dict(own_k=float(np.abs(TC1C2 - built).max()), TC1C2_clear=float(np.abs(TC1C2[clear] - g[prefix + 'TC1C2'][clear]).max()),
                k_differs_clear=int((k[clear] != ref_k[clear]).sum()), k_differs_tied=int((k[~clear] != ref_k[~clear]).sum()), n_tied=int((~clear).sum()),
                tied_excess=float((ref_rows[np.arange(len(k)), k] - ref_rows.min(1))[~clear].max()) if (~clear).any() else 0.0,
                sym_dists=float(np.abs(rows[finite] - ref_rows[finite]).max()),
                gap_clear=float(np.abs(gap[clear & np.isfinite(ref_gap)] - ref_gap[clear & np.isfinite(ref_gap)]).max(initial=0.0)))
    print(f'FIGURE stage1 {prefix}', figs)
    assert figs['own_k'] < DIST_TOL
    assert figs['k_differs_clear'] == 0 and figs['TC1C2_clear'] < DIST_TOL
    assert figs['tied_excess'] < NEAR
    assert np.array_equal(np.isfinite(rows), finite) and figs['sym_dists'] < DIST_TOL
    assert torch.equal(estimate_camera_poses_batch(cand, seeds, mesh_db, bsz=7), out['TC1C2'])


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_stage2_score_and_inliers(g, prefix):
    """The REFERENCE's TC1C2 in.  Distances (optional output) within 1e-5; n_inliers exactly and dists_sum within n_inliers x 1e-5 for
    every hypothesis the generator did not flag (a distance within 1e-4 of the threshold, or two conflicting inliers within 1e-4 of
    each other: at most 2 %).  The production launch (no table) gives the same bits as the one that writes the table."""
    from cosypose_amd.multiview_matching import score_hypotheses, score_tmaches_batch
    cand, _, mesh_db = rc.collections(g, prefix, 'cuda')
    tm = rc.tmatches_of(g, prefix)
    TC1C2 = dev(g[prefix + 'TC1C2'])
    n_inl, dsum, dists = score_hypotheses(cand, tm, TC1C2, mesh_db, THRESHOLD, return_dists=True)
    n_inl2, dsum2 = score_hypotheses(cand, tm, TC1C2, mesh_db, THRESHOLD)
    assert torch.equal(n_inl, n_inl2) and torch.equal(dsum, dsum2)
    assert torch.equal(score_tmaches_batch(cand, dict(tm), TC1C2, mesh_db, bsz=1000, seeds=rc.seeds_of(g, prefix)), dists)
    n_inl, dsum, dists = n_inl.cpu().numpy(), dsum.cpu().numpy(), dists.cpu().numpy()
    keep = ~g[prefix + 'excluded']
    ref_n, ref_sum = g[prefix + 'n_inliers'], g[prefix + 'dists_sum']
    figs = dict(dists=float(np.abs(dists - g[prefix + 'dists']).max()), left_out=f'{int((~keep).sum())} / {len(keep)}',
                n_inliers_differ=int((n_inl[keep] != ref_n[keep]).sum()), n_inliers_differ_left_out=int((n_inl[~keep] != ref_n[~keep]).sum()),
                dists_sum_over_bound=float((np.abs(dsum - ref_sum)[keep] / np.maximum(ref_n[keep], 1)).max()), max_n_inliers=int(ref_n.max()))
    print(f'FIGURE stage2 {prefix}', figs)
    assert (~keep).mean() <= 0.02
    assert figs['dists'] < DIST_TOL
    assert figs['n_inliers_differ'] == 0
    assert np.all(np.abs(dsum - ref_sum)[keep] <= ref_n[keep] * DIST_TOL)


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_stage3_best_per_view_pair(g, prefix):
    """The reference's distance table in (so n_inliers / dists_sum are its own): best_hypotheses and both inlier-match lists EXACTLY,
    hypothesis 0 never winning, the lowest id winning exact ties; with skip_hypothesis_0=False the first view pair comes back."""
    from cosypose_amd.multiview_matching import find_ransac_inliers, _Plan, _score
    seeds, tm = rc.seeds_of(g, prefix), rc.tmatches_of(g, prefix)
    args = (seeds['view1'], seeds['view2'], tm['hypothesis_id'], tm['cand1'], tm['cand2'], g[prefix + 'dists'], THRESHOLD, N_MIN_INLIERS)
    plan = _Plan(tm, torch.device('cuda'))
    n_inl, dsum, _ = _score(None, plan, None, THRESHOLD, dists_in=dev(g[prefix + 'dists']))
    assert np.array_equal(n_inl.cpu().numpy(), g[prefix + 'n_inliers'])
    assert np.array_equal(dsum.cpu().numpy(), g[prefix + 'dists_sum']), 'dists_sum is not added in the reference\'s order'
    out = find_ransac_inliers(*args)
    ref_best = g[prefix + 'best_hypotheses']
    ties = sum(int(((g[prefix + 'n_inliers'] == g[prefix + 'n_inliers'][h]) & (g[prefix + 'dists_sum'] == g[prefix + 'dists_sum'][h])
                    & (tm.hyp_pair == tm.hyp_pair[h])).sum() > 1) for h in ref_best)
    print(f'FIGURE stage3 {prefix}', dict(view_pairs=len(ref_best), winners_with_an_exact_tie=ties, inlier_matches=len(g[prefix + 'inlier_cand1'])))
    assert np.array_equal(out['best_hypotheses'], ref_best)
    assert np.array_equal(out['inlier_matches_cand1'], g[prefix + 'inlier_cand1'])
    assert np.array_equal(out['inlier_matches_cand2'], g[prefix + 'inlier_cand2'])
    assert np.array_equal(out['n_inliers'], g[prefix + 'n_inliers'][ref_best])
    assert all(v.dtype == np.int32 for k, v in out.items() if k != 'dists_sum')
    # without the reference's `hypothesis_id > 0` test: the plain rule, restated here on the fixture's table
    ref_n, ref_sum = g[prefix + 'n_inliers'], g[prefix + 'dists_sum']
    plain = []
    for p in range(len(tm.pair_view1)):
        ids = np.flatnonzero((tm.hyp_pair == p) & (ref_n >= N_MIN_INLIERS))
        if len(ids):
            plain.append(ids[np.lexsort((ids, ref_sum[ids], -ref_n[ids]))[0]])
    with0 = find_ransac_inliers(*args, skip_hypothesis_0=False)
    assert np.array_equal(with0['best_hypotheses'], plain) and np.array_equal([h for h in plain if h > 0], ref_best)
    none = find_ransac_inliers(*args[:-1], 10 ** 6)
    assert len(none['best_hypotheses']) == 0 and len(none['inlier_matches_cand1']) == 0


def rot_trans_error(T, truth):
    dR = T[:3, :3].astype(np.float64) @ truth[:3, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def check_against_reference_run(g, prefix, out, label):
    """what stages 4 and 5 compare: rows, partition, view pairs, scene_infos; -> the matching's pairs as {(view1, view2): row}"""
    f, s, p = out['filtered_candidates'], out['scene_infos'], out['pairs_TC1C2']
    assert np.array_equal(f.infos['cand_id'].values, g[prefix + 'e2e_cand_id'])
    assert rc.partition(f.infos['obj_id'].values) == rc.partition(g[prefix + 'e2e_obj_id']), f'{label}: another partition into objects'
    pairs = {(a, b): n for n, (a, b) in enumerate(zip(p.infos['view1'].tolist(), p.infos['view2'].tolist()))}
    assert set(pairs) == set(zip(g[prefix + 'e2e_view1'].tolist(), g[prefix + 'e2e_view2'].tolist())), f'{label}: another set of view pairs'
    key = lambda n, sc, l: sorted(zip(np.asarray(n).tolist(), np.round(np.asarray(sc, np.float64), 6).tolist(), np.asarray(l).tolist()))
    assert key(s['n_cand'], s['score'], [int(l[4:]) - 1 for l in s['label']]) == key(g[prefix + 'e2e_info_n_cand'], g[prefix + 'e2e_info_score'], g[prefix + 'e2e_info_label'])
    assert list(s.columns) == ['obj_id', 'score', 'label', 'n_cand'] and s['obj_id'].tolist() == list(range(len(s)))
    return pairs


@pytest.mark.parametrize('prefix', ['a_', 'c_', 'd_'])
def test_stage4_end_to_end_reference_seeds(g, prefix):
    """Reference seeds in, own hypotheses.  filtered_candidates rows / partition, the set of view pairs and scene_infos equal the
    reference's; per view pair the winner's n_inliers equals the reference's; the winner's TC1C2 against the scene's TRUE relative
    camera pose does not exceed the largest error among the reference's hypotheses that reach the winner's n_inliers by more than 1e-5."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching
    cand, _, mesh_db = rc.collections(g, prefix, 'cuda')
    seeds = rc.seeds_of(g, prefix)
    out = multiview_candidate_matching(cand, mesh_db, dist_threshold=THRESHOLD, n_ransac_iter=2000, n_min_inliers=N_MIN_INLIERS, seeds=seeds)
    pairs = check_against_reference_run(g, prefix, out, prefix)
    scene = rc.scene_of(g, prefix)
    view_row = {v: n for n, v in enumerate(scene['cam_view_id'].tolist())}
    TCW = np.linalg.inv(scene['cam_TWC'])
    TC1C2 = out['pairs_TC1C2'].TC1C2.cpu().numpy()
    worst = dict(rot=-np.inf, trans=-np.inf, rot_err=0.0, trans_err=0.0, n_inliers_differ=0)
    for n, (a, b) in enumerate(zip(g[prefix + 'e2e_view1'].tolist(), g[prefix + 'e2e_view2'].tolist())):
        row = pairs[(a, b)]
        rot, trans = rot_trans_error(TC1C2[row], TCW[view_row[a]] @ scene['cam_TWC'][view_row[b]])
        worst['rot'] = max(worst['rot'], rot - g[prefix + 'e2e_rot_ceiling'][n]); worst['trans'] = max(worst['trans'], trans - g[prefix + 'e2e_trans_ceiling'][n])
        worst['rot_err'] = max(worst['rot_err'], rot); worst['trans_err'] = max(worst['trans_err'], trans)
        worst['n_inliers_differ'] += int(out['inliers']['n_inliers'][row] != g[prefix + 'e2e_n_inliers'][n])
    print(f'FIGURE stage4 {prefix}', dict(view_pairs=len(pairs), objects=len(out['scene_infos']), worst_rot_over_ceiling=worst['rot'],
                                        worst_trans_over_ceiling=worst['trans'], worst_rot_err=worst['rot_err'], worst_trans_err=worst['trans_err'],
                                        ceilings=(float(g[prefix + 'e2e_rot_ceiling'].max()), float(g[prefix + 'e2e_trans_ceiling'].max())),
                                        n_inliers_differ=worst['n_inliers_differ'], times=[out[k] for k in ('time_models', 'time_score', 'time_misc')]))
    assert worst['n_inliers_differ'] == 0
    assert worst['rot'] <= DIST_TOL and worst['trans'] <= DIST_TOL
    assert list(out['filtered_candidates'].infos.columns) == ['view_id', 'label', 'score', 'cand_id', 'obj_id']
    assert out['pairs_TC1C2'].TC1C2.is_cuda and out['filtered_candidates'].poses.is_cuda


@pytest.mark.parametrize('prefix', ['a_', 'c_'])
def test_stage5_own_seeds(g, prefix):
    """make_ransac_infos of this package at 2000 iterations: every view pair of these two scenes is sampled exhaustively (asserted by the
    generator), so the set of hypotheses is the reference's and only their order differs: same partition, same view pairs."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching
    cand, _, mesh_db = rc.collections(g, prefix, 'cuda')
    out = multiview_candidate_matching(cand, mesh_db, dist_threshold=THRESHOLD, n_ransac_iter=2000, n_min_inliers=N_MIN_INLIERS)
    print(f'FIGURE stage5 {prefix}', dict(view_pairs=len(out['pairs_TC1C2']), objects=len(out['scene_infos']),
                                        times=[out[k] for k in ('time_models', 'time_score', 'time_misc')]))
    check_against_reference_run(g, prefix, out, prefix)


def chain_inputs(g, prefix):
    cand, cams, mesh_db = rc.collections(g, prefix, 'cuda')
    cand.infos['scene_id'] = 3
    cand.infos['group_id'] = 0
    cams.infos['scene_id'] = 3
    cams.infos['batch_im_id'] = np.arange(len(cams))
    return cand, cams, mesh_db


def test_stage6_chain_predict_scene_state(g):
    """MultiviewScenePredictor on scene 164 (float32 candidates, true obj_id withheld): the partition is the scene's ground truth, the
    output keys and columns are the reference's, ba_output has objects x views rows per group, the loss history is finite and its
    last entry is not above its first."""
    from cosypose_amd.multiview_predictor import MultiviewScenePredictor
    cand, cams, mesh_db = chain_inputs(g, 'c_')
    predictor = MultiviewScenePredictor(mesh_db.aabb(), mesh_db)
    corners = lambda m: [sorted(map(tuple, rows)) for rows in m.points.cpu().numpy().tolist()]
    assert corners(predictor.mesh_db_ransac) == corners(mesh_db) and predictor.mesh_db_ransac.points.is_cuda      # the fixture's points ARE box corners
    lo = mesh_db.points.min(1).values
    assert torch.equal(predictor.mesh_db_ransac.points[:, 7], lo) and torch.equal(predictor.mesh_db_ransac.points[:, 1], mesh_db.points.max(1).values)
    pred = predictor.predict_scene_state(cand, cams, ba_n_iter=100)
    assert {'cand_inputs', 'cand_matched', 'scene/objects', 'scene/cameras', 'ba_input', 'ba_output', 'ba_output+all_cand'} <= set(pred)
    matched = pred['cand_matched']
    truth = rc.scene_of(g, 'c_')['cand_obj_id'][matched.infos['cand_id'].values]
    assert len(matched) == len(cand) and rc.partition(matched.infos['obj_id'].values) == rc.partition(truth)
    objects, cameras, ba_out = pred['scene/objects'], pred['scene/cameras'], pred['ba_output']
    groups = sorted(set(objects.infos['view_group']))
    rows = sum(int((objects.infos['view_group'] == v).sum()) * int((cameras.infos['view_group'] == v).sum()) for v in groups)
    losses = [[float(l) for l in h['loss']] for h in pred['ba_history']]
    print('FIGURE stage6', dict(groups=len(groups), objects=len(objects), views=len(cameras), ba_output_rows=len(ba_out),
                                loss_first_last=[(l[0], l[-1], len(l)) for l in losses], matching_times=pred['matching']))
    assert len(ba_out) == rows == len(pred['ba_input']) and len(objects) == 12 and len(cameras) == 8
    assert list(ba_out.infos.columns) == ['scene_id', 'view_id', 'score', 'view_group', 'label', 'batch_im_id', 'obj_id', 'from_ba']
    assert ba_out.infos['from_ba'].all() and (ba_out.infos['score'] > 1).all() and ba_out.poses.shape == (rows, 4, 4)
    # object-major / view-minor, TCO = inv(TWC) TWO
    n_cam = len(cameras)
    assert ba_out.infos['obj_id'].tolist()[:n_cam] == [objects.infos['obj_id'][0]] * n_cam and ba_out.infos['view_id'].tolist()[:n_cam] == cameras.infos['view_id'].tolist()
    want = (torch.linalg.inv(cameras.TWC.double().cpu())[3] @ objects.TWO.double().cpu()[2]).cuda()
    assert (ba_out.poses[2 * n_cam + 3].double() - want).abs().max() < 1e-5
    assert {'scene_id', 'group_id', 'view_group'} <= set(objects.infos.columns) and {'scene_id', 'group_id', 'view_group'} <= set(cameras.infos.columns)
    assert len(pred['ba_output+all_cand']) == len(ba_out) + len(cand) and torch.isfinite(ba_out.poses).all()
    assert all(np.isfinite(l).all() and l[-1] <= l[0] for l in losses)


def test_known_camera_poses(g):
    """cameras given: one hypothesis per view pair from inv(TWC1) TWC2; the reference's test `hypothesis_id > 0` drops the first view
    pair, the keyword brings it back."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching
    cand, cams, mesh_db = rc.collections(g, 'k_', 'cuda')
    out = multiview_candidate_matching(cand, mesh_db, cameras=cams, dist_threshold=THRESHOLD, n_min_inliers=N_MIN_INLIERS)
    p = out['pairs_TC1C2']
    print('FIGURE known poses', dict(view_pairs=len(p), TC1C2=float(np.abs(p.TC1C2.cpu().numpy() - g['k_TC1C2']).max())))
    assert np.array_equal(out['inliers']['best_hypotheses'], g['k_best_hypotheses'])
    assert np.array_equal(p.infos['view1'].values, g['k_view1']) and np.array_equal(p.infos['view2'].values, g['k_view2'])
    assert np.abs(p.TC1C2.cpu().numpy() - g['k_TC1C2']).max() < DIST_TOL
    assert np.array_equal(out['filtered_candidates'].infos['cand_id'].values, g['k_cand_id'])
    assert rc.partition(out['filtered_candidates'].infos['obj_id'].values) == rc.partition(g['k_obj_id'])
    all_pairs = multiview_candidate_matching(cand, mesh_db, cameras=cams, dist_threshold=THRESHOLD, n_min_inliers=N_MIN_INLIERS, skip_hypothesis_0=False)
    assert len(all_pairs['pairs_TC1C2']) == len(p) + 1 and all_pairs['inliers']['best_hypotheses'][0] == 0


def test_nothing_reaches_n_min_inliers(g):
    """scene 161 (3 objects, 3 views): hypotheses exist, none has 3 inliers -- the reference returns nothing, and so does this."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching
    cand, _, mesh_db = rc.collections(g, 'e_', 'cuda')
    for seeds in (rc.seeds_of(g, 'e_'), None):
        out = multiview_candidate_matching(cand, mesh_db, n_ransac_iter=2000, seeds=seeds)
        assert len(out['filtered_candidates']) == 0 and out['filtered_candidates'].poses.shape == (0, 4, 4)
        assert list(out['filtered_candidates'].infos.columns) == ['view_id', 'label', 'score', 'cand_id', 'obj_id']
        assert len(out['pairs_TC1C2']) == 0 and out['pairs_TC1C2'].TC1C2.shape == (0, 4, 4)
        assert len(out['scene_infos']) == 0 and len(out['inliers']['best_hypotheses']) == 0


def test_two_runs_give_the_same_bits(g):
    from cosypose_amd.multiview_matching import estimate_camera_poses, score_hypotheses, multiview_candidate_matching
    cand, _, mesh_db = rc.collections(g, 'c_', 'cuda')
    seeds = rc.seeds_of(g, 'c_')
    h1, h2 = estimate_camera_poses(cand, seeds, mesh_db), estimate_camera_poses(cand, seeds, mesh_db)
    assert all(torch.equal(h1[k].view(torch.int32), h2[k].view(torch.int32)) for k in h1)
    runs = [multiview_candidate_matching(cand, mesh_db, n_ransac_iter=2000, seeds=seeds) for _ in range(2)]
    assert torch.equal(runs[0]['pairs_TC1C2'].TC1C2, runs[1]['pairs_TC1C2'].TC1C2)
    assert all(np.array_equal(runs[0]['inliers'][k], runs[1]['inliers'][k]) for k in runs[0]['inliers'])
    assert runs[0]['filtered_candidates'].infos.equals(runs[1]['filtered_candidates'].infos)


def test_float64_and_strided_inputs_and_batch_sizes(g):
    """float64 / non-contiguous poses and tables are narrowed once and give the bits of the float32 contiguous ones; model_bsz /
    score_bsz (nothing is stored per scoring, so there is nothing to batch) do not change a bit."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching
    from cosypose_amd.mesh_db import BatchedMeshes
    cand, _, mesh_db = rc.collections(g, 'a_', 'cuda')
    seeds = rc.seeds_of(g, 'a_')
    want = multiview_candidate_matching(cand, mesh_db, n_ransac_iter=2000, seeds=seeds)
    cand64, _, _ = rc.collections(g, 'a_', 'cuda')
    wide = torch.zeros(len(cand64), 4, 8, dtype=torch.float64, device='cuda')
    wide[:, :, ::2] = cand64.poses.double()
    cand64.poses = wide[:, :, ::2]
    assert not cand64.poses.is_contiguous()
    mesh64 = BatchedMeshes(mesh_db.infos, mesh_db.labels, mesh_db.points.double().transpose(1, 2).contiguous().transpose(1, 2), mesh_db.symmetries.double())
    for kwargs, c, m in ((dict(), cand64, mesh64), (dict(model_bsz=10, score_bsz=100), cand, mesh_db)):
        got = multiview_candidate_matching(c, m, n_ransac_iter=2000, seeds=seeds, **kwargs)
        assert torch.equal(got['pairs_TC1C2'].TC1C2, want['pairs_TC1C2'].TC1C2) and got['pairs_TC1C2'].TC1C2.dtype == torch.float32
        assert all(np.array_equal(got['inliers'][k], want['inliers'][k]) for k in want['inliers'])
        assert got['filtered_candidates'].infos.equals(want['filtered_candidates'].infos)
    assert got['filtered_candidates'].poses.dtype == cand.poses.dtype


def test_esize_past_the_documented_limit():
    """65 x 65 = 4225 tentative matches in one view pair > cosy_ransac_max_tmatches() = 4096: COSY_ESIZE (-4), not a wrong answer; 64 x 64
    = 4096, the limit itself, runs."""
    import pandas as pd
    from cosypose_amd._lib import CosyHipError
    from cosypose_amd.mesh_db import BatchedMeshes
    from cosypose_amd.multiview_matching import multiview_candidate_matching, max_tmatches
    from cosypose_amd.tensor_collection import PandasTensorCollection
    assert max_tmatches() == 4096
    labels = np.array(['obj_000001'])
    corners = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float32).mul(0.05)[None]
    mesh_db = BatchedMeshes({'obj_000001': dict(label='obj_000001', n_sym=1)}, labels, corners.cuda(), torch.eye(4)[None, None].cuda())

    def scene(n):
        poses = torch.eye(4).repeat(2 * n, 1, 1)
        poses[:, 0, 3] = torch.arange(2 * n) % n * 0.5         # candidate i of view 0 and of view 1 coincide; the others are 0.5 m apart
        poses[:, 2, 3] = 1.0
        infos = pd.DataFrame(dict(view_id=np.repeat([0, 1], n), label='obj_000001', score=1.0))
        # hypotheses 1 (pair 0 -> 1) and 2 (pair 1 -> 0) from two coinciding matches each: TC1C2 = identity, every candidate matched;
        # hypothesis 0 (which can never win) from matches that are 0.5 m off: one inlier fewer
        seeds = dict(view1=[0, 0, 1], view2=[1, 1, 0], match1_cand1=[0, 0, n], match1_cand2=[n + 1, n, 0], match2_cand1=[1, 1, n + 1], match2_cand2=[n + 2, n + 1, 1])
        return PandasTensorCollection(infos, poses=poses.cuda()), seeds
    cand, seeds = scene(65)
    with pytest.raises(CosyHipError, match=r'error -4.*4225'):
        multiview_candidate_matching(cand, mesh_db, seeds=seeds)
    cand, seeds = scene(64)
    out = multiview_candidate_matching(cand, mesh_db, seeds=seeds)
    assert out['inliers']['best_hypotheses'].tolist() == [1, 2] and out['inliers']['n_inliers'].tolist() == [64, 64]
    assert out['inliers']['inlier_matches_cand1'].tolist() == list(range(128)) and out['inliers']['inlier_matches_cand2'].tolist() == list(range(64, 128)) + list(range(64))
    assert len(out['filtered_candidates']) == 128 and len(out['scene_infos']) == 64 and len(out['pairs_TC1C2']) == 2
    assert torch.equal(out['pairs_TC1C2'].TC1C2.cpu(), torch.eye(4).repeat(2, 1, 1))
